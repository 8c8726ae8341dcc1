// checkpoint.bin of the host front end (host/terastructure_main.cpp: -checkpoint writes it, -resume reads it), in a header
// of its own with no HIP and no libtsamd in it, so that tests/test_checkpoint_format_cpu.py can drive it alone.
//
// One file, little-endian, every section a multiple of 8 bytes:
//   FileHeader   the CLI's magic and version; n, l, k, rfreq, the seed and the stop threshold of the run that wrote it; how
//                many shards (devices) that run had; the byte counts of the two engine parts; a checksum of this header and HostState
//   HostState    iter, the stop rule's prev_h / nh / max_h, the Mt19937 state with its index
//   loc part     tsamd_state_export's location part as exported by context 0 (identical on every shard)
//   indiv part   ONE individual part for all n individuals (shard_begin 0, shard_count n): the shards' parts joined, so
//                that a file written with one device count resumes with another (slice() cuts it on tsamd_shard_range's
//                boundaries)
// The engine parts carry their own headers and checksums (include/tsamd.h: BlobHeader mirrors tsamd_state_header; the
// front end asserts that the two agree).  The file is written to <path>.tmp and rename()d: a checkpoint.bin that exists
// is complete.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

namespace ckpt {

constexpr uint64_t kFileMagic = 0x3130544b43535454ull;  // "TTSCKT01"
constexpr uint32_t kFileVersion = 1;
constexpr uint32_t kBlobMagic = 0x54534d54u;  // TSAMD_STATE_MAGIC
constexpr uint32_t kBlobVersion = 1, kPartIndiv = 1, kPartLoc = 2;

struct BlobHeader {  // = tsamd_state_header
  uint32_t magic, version, part;
  uint32_t n, l, k, shard_begin, shard_count;
  uint32_t max_inner, reserved0;
  double alpha, eta0, eta1, nodetau0, nodekappa, conv_thresh, gamma_scale;
  uint64_t payload_bytes, checksum;
  uint64_t reserved1[2];
};
static_assert(sizeof(BlobHeader) == 128, "tsamd_state_header is 128 bytes");

struct FileHeader {
  uint64_t magic;
  uint32_t version, n, l, k, rfreq, nparts;
  double seed, stop_threshold;
  uint64_t loc_bytes, indiv_bytes;
  uint64_t head_checksum;  // FNV-1a (below) over this header with this field 0, followed by HostState
};
static_assert(sizeof(FileHeader) == 72, "no padding");

struct HostState {
  uint32_t iter, nh;
  double prev_h, max_h;
  uint32_t mt[624];
  int32_t mti;
  uint32_t reserved;
};
static_assert(sizeof(HostState) == 24 + 624 * 4 + 8, "no padding");

inline uint64_t fnv1a_words(const void *data, uint64_t bytes);
inline uint64_t head_checksum(FileHeader fh, const HostState &hs) {
  uint8_t both[sizeof fh + sizeof hs];
  fh.head_checksum = 0;
  memcpy(both, &fh, sizeof fh);
  memcpy(both + sizeof fh, &hs, sizeof hs);
  return fnv1a_words(both, sizeof both);
}

// where a Buf's bytes come from, if not from new[]: the front end hands its snapshots out of pinned host memory, which the
// engine fills by one DMA (get returns nullptr when it cannot; put may be called from another thread than get)
struct BufSource {
  void *(*get)(size_t bytes);
  void (*put)(void *p, size_t bytes);
};

// a byte buffer that is not zero-filled when it is made (hundreds of megabytes per snapshot)
struct Buf {
  uint8_t *p = nullptr;
  size_t n = 0;
  const BufSource *src = nullptr;
  Buf() = default;
  ~Buf() { release(); }
  Buf(Buf &&o) noexcept : p(o.p), n(o.n), src(o.src) { o.p = nullptr, o.n = 0, o.src = nullptr; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p, n = o.n, src = o.src;
      o.p = nullptr, o.n = 0, o.src = nullptr;
    }
    return *this;
  }
  Buf(const Buf &o) { *this = o; }
  Buf &operator=(const Buf &o) {  // (a copy is ordinary memory, whatever the original is)
    if (this != &o) {
      alloc(o.n);
      if (o.n) memcpy(p, o.p, o.n);
    }
    return *this;
  }
  // false: the source had no memory (the buffer is then empty)
  bool alloc(size_t bytes, const BufSource *from = nullptr) {
    release();
    p = from ? (uint8_t *)from->get(bytes ? bytes : 1) : new uint8_t[bytes ? bytes : 1];
    if (!p) return false;
    n = bytes;
    src = from;
    return true;
  }
  void release() {
    if (p && src)
      src->put(p, n ? n : 1);
    else
      delete[] p;
    p = nullptr, n = 0, src = nullptr;
  }
  uint8_t *data() { return p; }
  const uint8_t *data() const { return p; }
  size_t size() const { return n; }
};

// FNV-1a over little-endian 64-bit words (the checksum of include/tsamd.h); bytes past the last whole word are ignored
inline uint64_t fnv1a_words(const void *data, uint64_t bytes) {
  uint64_t h = 14695981039346656037ull;
  const uint8_t *p = (const uint8_t *)data;
  for (uint64_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    memcpy(&w, p + i, 8);
    h = (h ^ w) * 1099511628211ull;
  }
  return h;
}

// tsamd_shard_range's rule: contiguous shards of ceil(n / world) rounded up to a multiple of 4 individuals
inline void shard_range(uint32_t n, uint32_t rank, uint32_t world, uint32_t *begin, uint32_t *count) {
  if (world == 0) world = 1;
  uint64_t per = ((uint64_t)n + world - 1) / world;
  per = (per + 3) / 4 * 4;
  const uint64_t b = (uint64_t)rank * per < n ? (uint64_t)rank * per : n;
  const uint64_t e = b + per < n ? b + per : n;
  *begin = (uint32_t)b;
  *count = (uint32_t)(e - b);
}

inline uint64_t indiv_payload_bytes(uint64_t count, uint64_t k) { return 16 * count * k + (4 * count + 7) / 8 * 8; }

// header of an engine part: magic, version, which part, the byte count against its own shard and against the buffer, checksum
inline bool check_blob(const uint8_t *blob, uint64_t bytes, uint32_t part, const char *name, BlobHeader *out, std::string *err) {
  if (bytes < sizeof(BlobHeader)) return *err = std::string(name) + " part is shorter than its header", false;
  BlobHeader h;
  memcpy(&h, blob, sizeof h);
  if (h.magic != kBlobMagic || h.version != kBlobVersion) return *err = std::string(name) + " part: bad magic or version", false;
  if (h.part != part) return *err = std::string(name) + " part: it is the other part", false;
  if (h.payload_bytes != bytes - sizeof h) return *err = std::string(name) + " part: byte count does not match its header", false;
  if (part == kPartIndiv && h.payload_bytes != indiv_payload_bytes(h.shard_count, h.k))
    return *err = std::string(name) + " part: byte count does not match its shard", false;
  if (fnv1a_words(blob + sizeof h, h.payload_bytes) != h.checksum) return *err = std::string(name) + " part: bad checksum", false;
  if (out) *out = h;
  return true;
}

// the shards' individual parts (rank order, together covering 0 .. n) -> one part for all n individuals
inline bool merge_indiv(const std::vector<Buf> &parts, Buf *out, std::string *err) {
  if (parts.empty()) return *err = "no individual part", false;
  std::vector<BlobHeader> hs(parts.size());
  uint64_t next = 0;
  for (size_t i = 0; i < parts.size(); ++i) {
    if (!check_blob(parts[i].data(), parts[i].size(), kPartIndiv, "indiv", &hs[i], err)) return false;
    if (hs[i].shard_begin != next || hs[i].k != hs[0].k || hs[i].n != hs[0].n) return *err = "individual parts do not follow each other", false;
    next += hs[i].shard_count;
  }
  if (next != hs[0].n) return *err = "individual parts do not cover all individuals", false;
  const uint64_t n = hs[0].n, k = hs[0].k, pay = indiv_payload_bytes(n, k);
  out->alloc(sizeof(BlobHeader) + pay);
  uint8_t *g = out->data() + sizeof(BlobHeader), *w = g + 8 * n * k, *c = w + 8 * n * k;
  memset(c, 0, pay - 16 * n * k);  // (the padding behind an odd number of c_n)
  for (size_t i = 0; i < parts.size(); ++i) {
    const uint64_t b = hs[i].shard_begin, cnt = hs[i].shard_count;
    const uint8_t *src = parts[i].data() + sizeof(BlobHeader);
    memcpy(g + 8 * b * k, src, 8 * cnt * k);
    memcpy(w + 8 * b * k, src + 8 * cnt * k, 8 * cnt * k);
    memcpy(c + 4 * b, src + 16 * cnt * k, 4 * cnt);
  }
  BlobHeader h = hs[0];
  h.shard_begin = 0;
  h.shard_count = (uint32_t)n;
  h.payload_bytes = pay;
  h.checksum = fnv1a_words(g, pay);
  memcpy(out->data(), &h, sizeof h);
  return true;
}

// individuals [begin, begin + count) of a global individual part as a part of their own
inline bool slice_indiv(const uint8_t *global, uint64_t bytes, uint32_t begin, uint32_t count, Buf *out, std::string *err) {
  BlobHeader h;
  if (!check_blob(global, bytes, kPartIndiv, "indiv", &h, err)) return false;
  if (h.shard_begin != 0 || h.shard_count != h.n) return *err = "the file's individual part does not cover all individuals", false;
  if ((uint64_t)begin + count > h.n) return *err = "slice exceeds n", false;
  const uint64_t n = h.n, k = h.k, pay = indiv_payload_bytes(count, k);
  out->alloc(sizeof(BlobHeader) + pay);
  const uint8_t *g = global + sizeof(BlobHeader), *w = g + 8 * n * k, *c = w + 8 * n * k;
  uint8_t *dst = out->data() + sizeof(BlobHeader);
  memcpy(dst, g + 8 * (uint64_t)begin * k, 8 * (uint64_t)count * k);
  memcpy(dst + 8 * (uint64_t)count * k, w + 8 * (uint64_t)begin * k, 8 * (uint64_t)count * k);
  memset(dst + 16 * (uint64_t)count * k, 0, pay - 16 * (uint64_t)count * k);
  memcpy(dst + 16 * (uint64_t)count * k, c + 4 * (uint64_t)begin, 4 * (uint64_t)count);
  h.shard_begin = begin;
  h.shard_count = count;
  h.payload_bytes = pay;
  h.checksum = fnv1a_words(dst, pay);
  memcpy(out->data(), &h, sizeof h);
  return true;
}

// <path>.tmp, then rename(): `indiv` is the global part
inline bool write_file(const std::string &path, FileHeader fh, const HostState &hs, const uint8_t *loc, uint64_t loc_bytes,
                       const uint8_t *indiv, uint64_t indiv_bytes, std::string *err) {
  fh.magic = kFileMagic;
  fh.version = kFileVersion;
  fh.loc_bytes = loc_bytes;
  fh.indiv_bytes = indiv_bytes;
  fh.head_checksum = head_checksum(fh, hs);
  const std::string tmp = path + ".tmp";
  FILE *f = fopen(tmp.c_str(), "wb");
  if (!f) return *err = "cannot open " + tmp + ": " + strerror(errno), false;
  bool ok = fwrite(&fh, sizeof fh, 1, f) == 1 && fwrite(&hs, sizeof hs, 1, f) == 1 && fwrite(loc, 1, loc_bytes, f) == loc_bytes &&
            fwrite(indiv, 1, indiv_bytes, f) == indiv_bytes;
  ok = fflush(f) == 0 && ok;
  ok = fsync(fileno(f)) == 0 && ok;  // (the bytes are on the disk before the name is: a crash leaves no empty checkpoint.bin)
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    *err = "error writing " + tmp + ": " + strerror(errno);
    unlink(tmp.c_str());
    return false;
  }
  if (rename(tmp.c_str(), path.c_str()) != 0) return *err = "cannot rename " + tmp + ": " + strerror(errno), false;
  const size_t slash = path.rfind('/');  // (and the new name itself: the directory entry)
  const int dfd = open(slash == std::string::npos ? "." : slash == 0 ? "/" : path.substr(0, slash).c_str(), O_RDONLY | O_DIRECTORY);
  if (dfd >= 0) {
    (void)fsync(dfd);
    close(dfd);
  }
  return true;
}

// what a resumed run must have been started with
struct Expect {
  uint32_t n, l, k, rfreq;
  double seed;
};

// false with a message: cannot open, truncated, corrupt, or written by a run with other flags
inline bool read_file(const std::string &path, const Expect &want, FileHeader *fh, HostState *hs, Buf *loc, Buf *indiv, std::string *err) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) {
    *err = "cannot open " + path + ": " + strerror(errno);
    if (FILE *t = fopen((path + ".tmp").c_str(), "rb")) {
      fclose(t);
      *err += " (" + path + ".tmp exists: the run that wrote it ended before the checkpoint was complete; it is not used)";
    }
    return false;
  }
  auto bad = [&](const std::string &why) {
    fclose(f);
    *err = path + ": " + why;
    return false;
  };
  if (fread(fh, sizeof *fh, 1, f) != 1) return bad("truncated (no file header)");
  if (fh->magic != kFileMagic) return bad("not a checkpoint file (bad magic)");
  if (fh->version != kFileVersion) return bad("checkpoint format version " + std::to_string(fh->version) + " is not " + std::to_string(kFileVersion));
  // the header's own checksum before its fields are believed: a damaged header is "corrupt", not "written with -k ..."
  if (fread(hs, sizeof *hs, 1, f) != 1) return bad("truncated (host state)");
  if (head_checksum(*fh, *hs) != fh->head_checksum) return bad("corrupt (checksum of the file header and the host state)");
  if (fh->n != want.n) return bad("written with -n " + std::to_string(fh->n) + ", this run has -n " + std::to_string(want.n));
  if (fh->l != want.l) return bad("written with -l " + std::to_string(fh->l) + ", this run has -l " + std::to_string(want.l));
  if (fh->k != want.k) return bad("written with -k " + std::to_string(fh->k) + ", this run has -k " + std::to_string(want.k));
  if (memcmp(&fh->seed, &want.seed, sizeof(double)) != 0) return bad("written with -seed " + std::to_string(fh->seed) + ", this run has -seed " + std::to_string(want.seed));
  if (fh->rfreq != want.rfreq) return bad("written with -rfreq " + std::to_string(fh->rfreq) + ", this run has -rfreq " + std::to_string(want.rfreq));
  if (fseeko(f, 0, SEEK_END) != 0) return bad("cannot seek");
  const uint64_t size = (uint64_t)ftello(f), need = sizeof *fh + sizeof *hs + fh->loc_bytes + fh->indiv_bytes;
  if (fh->loc_bytes > (1ull << 46) || fh->indiv_bytes > (1ull << 46) || size != need)
    return bad("truncated or corrupt: " + std::to_string(size) + " bytes, its header says " + std::to_string(need));
  if (fseeko(f, (off_t)(sizeof *fh + sizeof *hs), SEEK_SET) != 0) return bad("cannot seek");
  if (hs->mti < 0 || hs->mti > 624) return bad("corrupt (index of the random number generator)");
  loc->alloc(fh->loc_bytes);
  indiv->alloc(fh->indiv_bytes);
  if (fread(loc->data(), 1, fh->loc_bytes, f) != fh->loc_bytes || fread(indiv->data(), 1, fh->indiv_bytes, f) != fh->indiv_bytes)
    return bad("truncated (engine state)");
  fclose(f);
  f = nullptr;
  BlobHeader bl, bi;
  std::string why;
  if (!check_blob(loc->data(), loc->size(), kPartLoc, "loc", &bl, &why) || !check_blob(indiv->data(), indiv->size(), kPartIndiv, "indiv", &bi, &why))
    return *err = path + ": corrupt: " + why, false;
  if (bl.n != fh->n || bl.l != fh->l || bl.k != fh->k || bi.n != fh->n || bi.l != fh->l || bi.k != fh->k || bi.shard_begin != 0 || bi.shard_count != fh->n)
    return *err = path + ": corrupt: the engine parts do not belong to the file header", false;
  return true;
}

// -project: the location part of a checkpoint, for a cohort of another size.  The same magic / version / checksum checks
// as read_file; l and k must be the file's, while n, the seed and rfreq are the training run's own business.  The individual
// part is not read (its bytes are counted: a truncated file is refused).  lambda [l][k][2] is the first array of the
// location part's payload (include/tsamd.h).
inline bool read_loc_part(const std::string &path, uint32_t l, uint32_t k, FileHeader *fh, Buf *loc, std::string *err) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return *err = "cannot open " + path + ": " + strerror(errno), false;
  auto bad = [&](const std::string &why) {
    fclose(f);
    *err = path + ": " + why;
    return false;
  };
  HostState hs;
  if (fread(fh, sizeof *fh, 1, f) != 1) return bad("truncated (no file header)");
  if (fh->magic != kFileMagic) return bad("not a checkpoint file (bad magic)");
  if (fh->version != kFileVersion) return bad("checkpoint format version " + std::to_string(fh->version) + " is not " + std::to_string(kFileVersion));
  if (fread(&hs, sizeof hs, 1, f) != 1) return bad("truncated (host state)");
  if (head_checksum(*fh, hs) != fh->head_checksum) return bad("corrupt (checksum of the file header and the host state)");
  if (fh->l != l) return bad("written with -l " + std::to_string(fh->l) + ", this run has -l " + std::to_string(l));
  if (fh->k != k) return bad("written with -k " + std::to_string(fh->k) + ", this run has -k " + std::to_string(k));
  if (fseeko(f, 0, SEEK_END) != 0) return bad("cannot seek");
  const uint64_t size = (uint64_t)ftello(f), need = sizeof *fh + sizeof hs + fh->loc_bytes + fh->indiv_bytes;
  if (fh->loc_bytes > (1ull << 46) || fh->indiv_bytes > (1ull << 46) || size != need)
    return bad("truncated or corrupt: " + std::to_string(size) + " bytes, its header says " + std::to_string(need));
  if (fseeko(f, (off_t)(sizeof *fh + sizeof hs), SEEK_SET) != 0) return bad("cannot seek");
  loc->alloc(fh->loc_bytes);
  if (fread(loc->data(), 1, fh->loc_bytes, f) != fh->loc_bytes) return bad("truncated (engine state)");
  fclose(f);
  f = nullptr;
  BlobHeader bl;
  std::string why;
  if (!check_blob(loc->data(), loc->size(), kPartLoc, "loc", &bl, &why)) return *err = path + ": corrupt: " + why, false;
  if (bl.n != fh->n || bl.l != fh->l || bl.k != fh->k) return *err = path + ": corrupt: the location part does not belong to the file header", false;
  if (bl.payload_bytes < 16ull * bl.l * bl.k) return *err = path + ": corrupt: the location part is shorter than its lambda", false;
  return true;
}

}  // namespace ckpt
