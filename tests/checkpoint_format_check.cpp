// Checker for host/checkpoint.h alone (compiled and run by tests/test_checkpoint_format_cpu.py, plain and under
// -fsanitize=address,undefined): synthetic engine parts -> checkpoint.bin -> read back; the global individual part
// re-sliced into 1, 2, 3 and 8 shards by tsamd_shard_range's rule and joined again; every refusal path.
// usage: checkpoint_format_check <dir>
#include <math.h>
#include <stdlib.h>

#include <string>
#include <utility>
#include <vector>

#include "checkpoint.h"

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED line %d: %s\n", __LINE__, #cond);         \
      failures++;                                              \
    }                                                          \
  } while (0)

static ckpt::Buf make_indiv(uint32_t n, uint32_t l, uint32_t k, uint32_t begin, uint32_t count) {
  ckpt::Buf b;
  const uint64_t pay = ckpt::indiv_payload_bytes(count, k);
  b.alloc(sizeof(ckpt::BlobHeader) + pay);
  memset(b.data(), 0, b.size());
  uint8_t *p = b.data() + sizeof(ckpt::BlobHeader);
  for (uint64_t i = 0; i < (uint64_t)count * k; ++i) {
    const double g = 1.0 + (double)((begin * (uint64_t)k + i) % 977) * 0.125, w = 1.0 / g;  // values that tell the individual and the array
    memcpy(p + 8 * i, &g, 8);
    memcpy(p + 8 * ((uint64_t)count * k + i), &w, 8);
  }
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t c = 7u * (begin + i) + 1u;
    memcpy(p + 16 * (uint64_t)count * k + 4 * (uint64_t)i, &c, 4);
  }
  ckpt::BlobHeader h;
  memset(&h, 0, sizeof h);
  h.magic = ckpt::kBlobMagic, h.version = ckpt::kBlobVersion, h.part = ckpt::kPartIndiv;
  h.n = n, h.l = l, h.k = k, h.shard_begin = begin, h.shard_count = count, h.max_inner = 10;
  h.alpha = 1.0 / k, h.eta0 = h.eta1 = 1.0, h.nodetau0 = 2.0, h.nodekappa = 0.5, h.conv_thresh = 1e-3, h.gamma_scale = l;
  h.payload_bytes = pay;
  h.checksum = ckpt::fnv1a_words(p, pay);
  memcpy(b.data(), &h, sizeof h);
  return b;
}

static ckpt::Buf make_loc(uint32_t n, uint32_t l, uint32_t k) {
  ckpt::Buf b;
  const uint64_t pay = 32ull * l * k + 32 + 32ull * k + 8 + 8 * 128;
  b.alloc(sizeof(ckpt::BlobHeader) + pay);
  memset(b.data(), 0, b.size());
  uint8_t *p = b.data() + sizeof(ckpt::BlobHeader);
  for (uint64_t i = 0; i < pay / 8; ++i) {
    const double v = 0.5 + (double)(i % 1013);
    memcpy(p + 8 * i, &v, 8);
  }
  ckpt::BlobHeader h;
  memset(&h, 0, sizeof h);
  h.magic = ckpt::kBlobMagic, h.version = ckpt::kBlobVersion, h.part = ckpt::kPartLoc;
  h.n = n, h.l = l, h.k = k, h.shard_begin = 0, h.shard_count = n, h.max_inner = 10;
  h.payload_bytes = pay;
  h.checksum = ckpt::fnv1a_words(p, pay);
  memcpy(b.data(), &h, sizeof h);
  return b;
}

static bool same(const ckpt::Buf &a, const ckpt::Buf &b) { return a.size() == b.size() && memcmp(a.data(), b.data(), a.size()) == 0; }

static std::vector<uint8_t> slurp(const std::string &path) {
  std::vector<uint8_t> out;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return out;
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return out;
}
static void spit(const std::string &path, const std::vector<uint8_t> &v, size_t bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (f) {
    fwrite(v.data(), 1, bytes, f);
    fclose(f);
  }
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  const uint32_t n = 1003, l = 37, k = 5;  // (odd n and k: an odd number of c_n, shards that end off a multiple of 4)
  // FNV-1a over words against the byte-wise definition on one word, and the ignored tail
  {
    const uint64_t w = 0x0123456789abcdefull;
    CHECK(ckpt::fnv1a_words(&w, 8) == (14695981039346656037ull ^ w) * 1099511628211ull);
    CHECK(ckpt::fnv1a_words(&w, 0) == 14695981039346656037ull);
  }
  // shard_range: the documented examples of tsamd_shard_range
  {
    uint32_t b, c;
    ckpt::shard_range(1000000, 7, 8, &b, &c);
    CHECK(b == 875000 && c == 125000);
    ckpt::shard_range(1003, 2, 3, &b, &c);
    CHECK(b == 672 && c == 331);
    ckpt::shard_range(5, 3, 8, &b, &c);
    CHECK(b == 5 && c == 0);
  }
  const ckpt::Buf whole = make_indiv(n, l, k, 0, n), loc = make_loc(n, l, k);
  std::string err;
  // slice into `world` shards, compare with parts made directly, join again
  for (uint32_t world : {1u, 2u, 3u, 8u}) {
    std::vector<ckpt::Buf> parts;
    for (uint32_t r = 0; r < world; ++r) {
      uint32_t b, c;
      ckpt::shard_range(n, r, world, &b, &c);
      ckpt::Buf s;
      CHECK(ckpt::slice_indiv(whole.data(), whole.size(), b, c, &s, &err));
      CHECK(same(s, make_indiv(n, l, k, b, c)));
      CHECK(ckpt::check_blob(s.data(), s.size(), ckpt::kPartIndiv, "indiv", nullptr, &err));
      parts.push_back(std::move(s));
    }
    ckpt::Buf joined;
    CHECK(ckpt::merge_indiv(parts, &joined, &err));
    CHECK(same(joined, whole));
    if (world > 1) {  // a missing shard, shards out of order
      std::vector<ckpt::Buf> fewer;
      for (uint32_t r = 0; r + 1 < world; ++r) {
        uint32_t b, c;
        ckpt::shard_range(n, r, world, &b, &c);
        fewer.push_back(make_indiv(n, l, k, b, c));
      }
      CHECK(!ckpt::merge_indiv(fewer, &joined, &err) && err.find("cover") != std::string::npos);
      std::swap(parts[0], parts[1]);
      CHECK(!ckpt::merge_indiv(parts, &joined, &err));
    }
  }
  {
    ckpt::Buf s;
    CHECK(!ckpt::slice_indiv(whole.data(), whole.size(), 1000, 4, &s, &err));                       // past n
    const ckpt::Buf part = make_indiv(n, l, k, 4, 100);
    CHECK(!ckpt::slice_indiv(part.data(), part.size(), 4, 10, &s, &err));                           // not a global part
    CHECK(!ckpt::check_blob(loc.data(), loc.size(), ckpt::kPartIndiv, "indiv", nullptr, &err));      // the other part
    CHECK(!ckpt::check_blob(whole.data(), whole.size() - 8, ckpt::kPartIndiv, "indiv", nullptr, &err));
    CHECK(!ckpt::check_blob(whole.data(), 64, ckpt::kPartIndiv, "indiv", nullptr, &err));
  }
  // the file: write, read back
  const std::string path = dir + "/checkpoint.bin";
  ckpt::FileHeader fh{};
  fh.n = n, fh.l = l, fh.k = k, fh.rfreq = 500, fh.nparts = 2, fh.seed = 1234.0, fh.stop_threshold = 1e-5;
  ckpt::HostState hs{};
  hs.iter = 1550, hs.nh = 2, hs.prev_h = -0.731, hs.max_h = -0.73;
  for (int i = 0; i < 624; ++i) hs.mt[i] = 2654435761u * (uint32_t)(i + 1);
  hs.mti = 17;
  CHECK(ckpt::write_file(path, fh, hs, loc.data(), loc.size(), whole.data(), whole.size(), &err));
  CHECK(fopen((path + ".tmp").c_str(), "rb") == nullptr);  // renamed
  const ckpt::Expect want{n, l, k, 500, 1234.0};
  ckpt::FileHeader fh2;
  ckpt::HostState hs2;
  ckpt::Buf loc2, ind2;
  CHECK(ckpt::read_file(path, want, &fh2, &hs2, &loc2, &ind2, &err));
  CHECK(fh2.nparts == 2 && fh2.stop_threshold == 1e-5 && memcmp(&hs, &hs2, sizeof hs) == 0 && same(loc, loc2) && same(whole, ind2));
  // refusals: other flags
  {
    ckpt::Expect w2 = want;
    w2.k = 4;
    CHECK(!ckpt::read_file(path, w2, &fh2, &hs2, &loc2, &ind2, &err) && err.find("-k 5") != std::string::npos);
    w2 = want, w2.seed = 99.0;
    CHECK(!ckpt::read_file(path, w2, &fh2, &hs2, &loc2, &ind2, &err) && err.find("-seed") != std::string::npos);
    w2 = want, w2.n = 1000;
    CHECK(!ckpt::read_file(path, w2, &fh2, &hs2, &loc2, &ind2, &err) && err.find("-n ") != std::string::npos);
    w2 = want, w2.l = 38;
    CHECK(!ckpt::read_file(path, w2, &fh2, &hs2, &loc2, &ind2, &err) && err.find("-l ") != std::string::npos);
    w2 = want, w2.rfreq = 1000;
    CHECK(!ckpt::read_file(path, w2, &fh2, &hs2, &loc2, &ind2, &err) && err.find("-rfreq") != std::string::npos);
  }
  // refusals: truncated, corrupted in each section, not a checkpoint, missing with a .tmp beside it
  const std::vector<uint8_t> bytes = slurp(path);
  CHECK(bytes.size() == sizeof(ckpt::FileHeader) + sizeof(ckpt::HostState) + loc.size() + whole.size());
  const std::string bad = dir + "/bad.bin";
  for (size_t cut : {(size_t)100, (size_t)1, bytes.size() - 10, bytes.size() - sizeof(ckpt::FileHeader) - 3}) {
    spit(bad, bytes, bytes.size() - cut);
    CHECK(!ckpt::read_file(bad, want, &fh2, &hs2, &loc2, &ind2, &err) && err.find("truncated") != std::string::npos);
  }
  const size_t at[] = {3, 40, sizeof(ckpt::FileHeader) + 100, sizeof(ckpt::FileHeader) + sizeof(ckpt::HostState) + 20,
                       sizeof(ckpt::FileHeader) + sizeof(ckpt::HostState) + 4000, bytes.size() - 9};
  for (size_t pos : at) {
    std::vector<uint8_t> v = bytes;
    v[pos] ^= 0x20;
    spit(bad, v, v.size());
    CHECK(!ckpt::read_file(bad, want, &fh2, &hs2, &loc2, &ind2, &err));
  }
  // a damaged field of the file header is reported as corruption, not as a run with other flags (the -k field: bytes 20..23)
  {
    std::vector<uint8_t> v = bytes;
    v[20] ^= 0x01;
    spit(bad, v, v.size());
    CHECK(!ckpt::read_file(bad, want, &fh2, &hs2, &loc2, &ind2, &err) && err.find("corrupt") != std::string::npos && err.find("-k") == std::string::npos);
  }
  CHECK(!ckpt::read_file(dir + "/none.bin", want, &fh2, &hs2, &loc2, &ind2, &err) && err.find("cannot open") != std::string::npos);
  spit(dir + "/gone.bin.tmp", bytes, bytes.size());
  CHECK(!ckpt::read_file(dir + "/gone.bin", want, &fh2, &hs2, &loc2, &ind2, &err) && err.find(".tmp exists") != std::string::npos);
  CHECK(!ckpt::write_file(dir + "/no/such/dir/checkpoint.bin", fh, hs, loc.data(), loc.size(), whole.data(), whole.size(), &err));
  // a Buf from a source of its own: taken once, given back once with its byte count (also when moved), a copy is ordinary
  // memory, and a source without memory leaves the buffer empty
  {
    static int taken = 0, given = 0;
    static size_t given_bytes = 0;
    static const ckpt::BufSource src = {[](size_t b) -> void * { return ++taken, malloc(b); },
                                        [](void *q, size_t b) { ++given, given_bytes = b, free(q); }};
    static const ckpt::BufSource none = {[](size_t) -> void * { return nullptr; }, [](void *, size_t) { ++given; }};
    {
      ckpt::Buf a;
      CHECK(a.alloc(100, &src) && a.size() == 100);
      memset(a.data(), 7, 100);
      ckpt::Buf b = std::move(a);
      ckpt::Buf c = b;
      CHECK(a.size() == 0 && b.size() == 100 && same(b, c) && taken == 1 && given == 0);
      ckpt::Buf d;
      CHECK(!d.alloc(100, &none) && d.size() == 0 && d.data() == nullptr);
    }
    CHECK(taken == 1 && given == 1 && given_bytes == 100);
  }
  printf("checkpoint format: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
