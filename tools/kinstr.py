#!/usr/bin/env python3
"""Static instruction counts of one kernel in a device assembly file (hipcc -save-temps): vector instructions in all,
the moves, the selects, and the literals the moves materialise most often.  A resident kernel's lone wave pays for every
vector instruction it issues (tools/ubench/op_cost.hip), so these counts are what its arithmetic-free work costs.
usage: tools/kinstr.py file.s 'ts_schedule<8, false, 0>' [--sections]
--sections: split the kernel's text at its s_memrealtime reads (a -DTSAMD_SCHED_TIME build: the in-kernel timers
bracket the gamma step, the sweeps, the folds, the exchanges and the epilogues) and count each stretch."""
import collections
import re
import subprocess
import sys


def kernel_text(path, want):
    """lines of the kernel whose demangled name contains `want`: from its label to its s_endpgm-terminated end"""
    lines = open(path, errors="replace").read().splitlines()
    labels = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+):", l)] if m]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in labels), capture_output=True, text=True).stdout.splitlines()
    for (i, _), name in zip(labels, names):
        if want in name and "(" in name:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            return lines[i + 1:end]
    raise SystemExit(f"no kernel matching {want!r} in {path}")


def count(lines):
    ops = collections.Counter()
    lits = collections.Counter()
    for l in lines:
        l = l.split(";")[0].strip()
        if not l or l.endswith(":") or l.startswith("."):
            continue
        parts = l.replace(",", " ").split()
        ops[parts[0]] += 1
        if parts[0] == "v_mov_b32_e32" and len(parts) >= 3 and not parts[2].startswith(("v", "s", "a", "ttmp", "exec", "vcc")):
            lits[parts[2]] += 1
    vec = sum(n for o, n in ops.items() if o.startswith("v_"))
    sel = sum(n for o, n in ops.items() if o.startswith("v_cndmask"))
    return {"all": sum(ops.values()), "vector": vec, "v_mov_b32": ops["v_mov_b32_e32"], "v_cndmask": sel,
            "v_accvgpr": sum(n for o, n in ops.items() if o.startswith("v_accvgpr")), "literals": lits.most_common(4)}


def main():
    path, want = sys.argv[1], sys.argv[2]
    text = kernel_text(path, want)
    c = count(text)
    print(f"{want}: {c['vector']} vector instructions of {c['all']}; v_mov_b32 {c['v_mov_b32']}, v_cndmask {c['v_cndmask']}, "
          f"v_accvgpr moves {c['v_accvgpr']}; moved literals: " + ", ".join(f"{v} x{n}" for v, n in c["literals"]))
    if "--sections" in sys.argv:
        cuts = [i for i, l in enumerate(text) if "s_memrealtime" in l]
        for n, (a, b) in enumerate(zip([0] + cuts, cuts + [len(text)])):
            s = count(text[a:b])
            if s["vector"] >= 100:
                print(f"  stretch {n:3d} (lines {a}-{b}): vector {s['vector']:5d}, v_mov_b32 {s['v_mov_b32']:4d}, v_cndmask {s['v_cndmask']:3d}; "
                      + ", ".join(f"{v} x{k}" for v, k in s["literals"]))


if __name__ == "__main__":
    main()
