"""Records what a build of libtsamd.so decides about launch modes and geometries, as a fixture for the CPU test of
csrc/tsamd_plan.h (tests/test_launch_plan_cpu.py, tests/golden/launch_plan_parent.json).

    TSAMD_LIB=<libtsamd.so of the commit to record> python tools/dump_launch_plans.py --commit <sha> --out <file.json>

Needs a GPU.  Every context is created with l = 2, so it costs only its weights; at most 16 are open at a time.  Per context
the file holds the facts the plan depends on and everything tsamd_launch_info, tsamd_schedule_geometry (both modes, or the
refusal) and tsamd_holblock_info report.  The occupancy answers of the kernels are not part of the ABI: they are read
through the library's C++ symbols -- the per-K ops objects (csrc/tsamd_unit.h), or, in a build from before those, the
*_blocks_per_cu_k<K> functions."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = [1, 3, 8, 9, 14, 16, 20, 22, 24, 32, 40]
NS = [200, 2_000, 10_000, 100_000, 1_048_576, 2_097_152]
KNOB_VARS = ["TSAMD_BLOCK", "TSAMD_GRID", "TSAMD_GRID_FIRST", "TSAMD_FIRST_VEC", "TSAMD_RESIDENT", "TSAMD_PERSISTENT",
             "TSAMD_HYBRID", "TSAMD_SCHED_WORKGROUPS", "TSAMD_TEST_MAX_WORKGROUPS"]
VARIANTS = [({"TSAMD_GRID": "64"}, {}), ({"TSAMD_RESIDENT": "0"}, {}), ({"TSAMD_PERSISTENT": "0"}, {}),
            ({"TSAMD_HYBRID": "0"}, {}), ({}, {"nodekappa": 0.7}), ({}, {"max_inner": 1}), ({}, {"max_inner": 201})]
WORLDS = [(40_000, 8), (1_800, 8), (1_000_000, 20), (250_000, 20)]


def occupancy(h, k):
    """The seven occupancy answers for K = k (all 0 above the K-specialised kernels)."""
    if k > 32:
        return {"first": [0, 0], "resident": 0, "schedule": 0, "holblock": 0, "hybrid": 0, "hybhol": 0}
    fn0, fn1 = C.CFUNCTYPE(C.c_int), C.CFUNCTYPE(C.c_int, C.c_int)

    def sym(name, suffix):
        return f"_ZN5tsamd{len(name)}{name}{suffix}"

    class PassOps(C.Structure):
        _fields_ = [("launch", C.c_void_p), ("first", fn1), ("resident", fn0)]

    class WholeOps(C.Structure):
        _fields_ = [("launch", C.c_void_p), ("blocks_per_cu", fn0), ("batch", C.c_int)]

    out = {}
    try:
        ops = PassOps.in_dll(h, sym(f"pass_ops_k{k}", "E"))
        out["first"] = [ops.first(1), ops.first(2)]
        out["resident"] = ops.resident()
        for fam in ("schedule", "holblock", "hybrid", "hybhol"):
            out[fam] = WholeOps.in_dll(h, sym(f"{fam}_ops_k{k}", "E")).blocks_per_cu()
    except ValueError:  # a build from before the ops objects
        first = fn1((sym(f"first_blocks_per_cu_k{k}", "Ei"), h))
        out["first"] = [first(1), first(2)]
        for fam in ("resident", "schedule", "holblock", "hybrid", "hybhol"):
            out[fam] = fn0((sym(f"{fam}_blocks_per_cu_k{k}", "Ev"), h))()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import torch

    from terastructure_amd import _lib

    h = _lib.load()
    vp, u32 = C.c_void_p, C.c_uint32

    def check(rc, ctx=None):
        if rc != 0:
            raise RuntimeError(h.tsamd_last_error(ctx).decode())

    def create(n, k, world=1, rank=0, **over):
        cfg = _lib.Config()
        h.tsamd_default_config(C.byref(cfg), n, 2, k)
        cfg.world, cfg.rank = world, rank
        for name, v in over.items():
            setattr(cfg, name, v)
        ctx = vp()
        check(h.tsamd_create(C.byref(cfg), C.byref(ctx)))
        return cfg, ctx

    def record(cfg, ctx, env, exchange, share):
        kps, grid, gfirst = u32(), u32(), u32()
        check(h.tsamd_launch_info(ctx, C.byref(kps), C.byref(grid), C.byref(gfirst)), ctx)
        geo = {}
        for name, mode in (("per_snp", _lib.LAUNCH_PER_SNP), ("per_schedule", _lib.LAUNCH_PER_SCHEDULE)):
            v = [u32() for _ in range(4)]
            rc = h.tsamd_schedule_geometry(ctx, mode, *[C.byref(x) for x in v])
            geo[name] = [x.value for x in v] if rc == 0 else None  # [workgroups, per thread, exchange levels, on chip]
        batch = u32()
        check(h.tsamd_holblock_info(ctx, C.byref(batch), None, None), ctx)
        return {"n": cfg.n, "k": cfg.k, "world": cfg.world, "rank": cfg.rank, "max_inner": cfg.max_inner, "nodekappa": cfg.nodekappa,
                "flags": cfg.flags, "device_share": share, "exchange": exchange, "env": dict(env),
                "kernels_per_snp": kps.value, "grid": grid.value, "grid_first": gfirst.value, "geometry": geo, "batch": batch.value}

    for v in KNOB_VARS + ["TSAMD_DEVICE_SHARE"]:
        os.environ.pop(v, None)
    entries = []
    for k in KS:
        for n in NS:
            cfg, ctx = create(n, k)
            entries.append(record(cfg, ctx, {}, "none", 1))
            h.tsamd_destroy(ctx)
    for env, over in VARIANTS:
        os.environ.update(env)
        cfg, ctx = create(100_000, 8, **over)
        entries.append(record(cfg, ctx, env, "none", 1))
        h.tsamd_destroy(ctx)
        for v in env:
            del os.environ[v]
    for n, k in WORLDS:
        for world in (2, 3, 4):
            made = [create(n, k, world, r) for r in range(world)]
            arr = (vp * world)(*[ctx for _, ctx in made])
            check(h.tsamd_p2p_connect_local(arr, world), made[0][1])
            for cfg, ctx in made:
                entries.append(record(cfg, ctx, {}, "p2p", world))
            for _, ctx in made:
                h.tsamd_destroy(ctx)
    doc = {"commit": args.commit, "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "occupancy": {str(k): occupancy(h, k) for k in sorted(set(KS) | {8, 20})}, "entries": entries}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(entries)} contexts recorded in {args.out}")


if __name__ == "__main__":
    main()
