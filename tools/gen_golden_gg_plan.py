"""Writes tests/golden/gg_plan_parent.json: what the gather-GEMM side queries vg_gather_gemm_nparts / _tile_m / _ws_bytes /
_family and the plan query vg_gather_gemm_plan answered, per geometry, BEFORE the wrappers were moved onto the one plan
record (ABI 21 deleted the four side queries), and what vg_bn_finalize_act_forward_supported answered for the shape table
of tests/test_bn_cpu.py.  tests/test_gg_cpu.py and tests/test_bn_cpu.py assert that the record reproduces all of it.

It was run ONCE, at commit 31d8a42 ("Exact-arithmetic tests for the BatchNorm kernels; launch-plan query", ABI 20), on
the built library, host only (no GPU):

    python tools/gen_golden_gg_plan.py

It CANNOT be re-run on a later checkout: the exports it records are gone.  It stays as the record of how the fixture was
made -- which descriptor each query saw:

  nparts        ops.gather_gemm's protocol: a launch that emits statistics asks vg_gather_gemm_nparts with a non-NULL
                `stats` (and its bias), before activation, mask and workspace are set; a launch without statistics has 0
  ws_bytes      the launch's descriptor (bias, statistics, activation, mask) without a workspace
  family        the same descriptor with the workspace of ws_bytes attached
  tile_m        the launch's descriptor
  tile_m_stats  ops.gather_gemm_tile_m's protocol (engine.can_group, the layerwise test): non-NULL `stats`, nothing else
  plan          ops.gather_gemm_plan(g, dtype, bias, want_stats, act, mask): placeholder workspace and the zero page

Rows added to tests/_gg_ref.ALL_CASES after ABI 20 (the mask row of ggp<4> and the sub-pixel row of ggp<2,32> that came with
csrc/conv_epilogue.hpp) have no side query to record: their entries hold the plan the library of the commit BEFORE the row
answered (nparts, tile_m = bm, ws_bytes, family = timing_family from that plan; tile_m_stats = bm of the want_stats plan).
add_rows() below writes them, with the library of that commit selected and nothing else touched:

    VG_LIB_PATH=<libvaegan_hip.so built from the commit before the rows> python tools/gen_golden_gg_plan.py --add-rows

Geometries: every row of tests/_gg_ref.ALL_CASES under its own switches, and under the default switches every launch of
the three networks at the benchmarked shapes (tests/_gg_ref.network_launches).  "can_group" holds, per shape, the tile
rows of every BatchNorm stage of the Discriminator at 2B and the answer the condition of engine.StackEngine.can_group(B, 2)
gives from them (every slab inside one group).
"""
import json
import os
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vae-gan-based-model-for-image-generation-and-denoising_amd"
OUT = os.path.join(ROOT, "tests", "golden", "gg_plan_parent.json")
SOME = 64                                   # non-NULL, 16-byte aligned; the queries never dereference a pointer


def desc(L, g, bias=False, stats=False, act=None, mask=None, ws_bytes=0):
    d = L.GGDesc(X=SOME, W=SOME, Y=SOME, bias=SOME if bias else 0, stats=SOME if stats else 0, zeros=SOME, B=g.B, GH=g.GH,
                 GW=g.GW, IH=g.IH, IW=g.IW, IC=g.IC, SY=g.SY, SX=g.SX, DY=g.DY, DX=g.DX, TH=g.TH, TW=g.TW, y0=L.i4(g.y0),
                 x0=L.i4(g.x0), N=g.N, Kp=g.Kp, OH=g.OH, OW=g.OW, OC=g.OC, OSY=g.OSY, OSX=g.OSX, ooy=L.i4(g.ooy),
                 oox=L.i4(g.oox), nphase=g.nphase)
    if act is not None:
        d.act, d.act_slope = act
    if mask is not None:
        d.mask_x, d.mask_act, d.mask_slope = SOME, mask[0], mask[1]
    if ws_bytes:
        d.ws, d.ws_bytes = SOME, ws_bytes
    return d


def ask(fn, d, dtype):
    r = fn(byref(d), dtype)
    assert r >= 0, (fn.__name__, r)
    return int(r)


def record(L, ops, g, dtype, bias, want_stats, act, mask):
    lib = L.load()
    launch = desc(L, g, bias, want_stats, act, mask)
    nparts = ask(lib.vg_gather_gemm_nparts, desc(L, g, bias, True), dtype) if want_stats else 0
    ws_bytes = ask(lib.vg_gather_gemm_ws_bytes, launch, dtype)
    family = ask(lib.vg_gather_gemm_family, desc(L, g, bias, want_stats, act, mask, ws_bytes), dtype)
    plan = ops.gather_gemm_plan(g, dtype, bias=bias, want_stats=want_stats, act=act, mask=mask)
    plan["detail"] = list(plan["detail"])
    return dict(nparts=nparts, tile_m=ask(lib.vg_gather_gemm_tile_m, launch, dtype),
                tile_m_stats=ask(lib.vg_gather_gemm_tile_m, desc(L, g, stats=True), dtype), ws_bytes=ws_bytes, family=family,
                plan=plan)


def bn_shape_table(ops, B):
    """(slab rows per group, groups, C, rows, dtype, VG_BN_FUSED_FWD) of tests/test_bn_cpu.py's one-launch table."""
    rows = [(nparts, groups, C, rpg * groups, B.BF16, 1) for _, rpg, groups, C, nparts, _, _ in B.FUSED_CASES]
    rows += [(nparts, groups, C, rpg * groups, B.BF16, 1) for pair in B.FUSED_REFUSED.values() for rpg, groups, C, nparts in pair]
    rows += [(3, 1, 64, 144, B.F32, 1), (3, 1, 64, 144, B.BF16, 0)]
    for _, rpg, groups, C, _, _ in B.CHAIN_CASES:
        n = ops.bn_launch_plan("reduce", rpg * groups, C, B.BF16, groups)["blocks_per_group"]
        rows.append((n, groups, C, rpg * groups, B.BF16, 1))
    return rows


def main() -> None:
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from importlib import import_module
    import _bn_ref as B
    import _gg_ref as R
    L, ops = import_module(PKG + "._lib"), import_module(PKG + ".ops")
    lib = L.load()
    assert lib.vg_abi_version() == 20, "the side queries exist at ABI 20 only"
    switch_names = sorted({n for c in R.ALL_CASES for n in c.switches} | {"VG_BN_FUSED_FWD"})

    def switches(env):
        for n in switch_names:
            os.environ.pop(n, None)
        os.environ.update(env)
        ops.reload_switches()

    out = dict(parent="31d8a42", cases={}, networks={}, can_group={}, bn_fused=[])
    for c in R.ALL_CASES:
        switches(c.switches)
        out["cases"][c.id] = record(L, ops, c.specs()[0], c.dtype, c.has("b"), c.has("s"), c.act, c.mask)
    switches({})
    for S, nb, dtype in R.NETWORK_SHAPES:
        shape = f"S{S}_B{nb}_{dtype}"
        out["networks"][shape] = {key: record(L, ops, g, kdt, **epi) for key, g, kdt, epi in R.network_launches(S, nb, dtype)}
        stages, answer = [], True
        for i, g, kdt, rows_per_group, plain in R.group_stages(S, nb, dtype):
            bm = ask(lib.vg_gather_gemm_tile_m, desc(L, g, stats=True), kdt)
            stages.append(dict(stage=i, bm=bm, rows_per_group=rows_per_group, plain=plain))
            answer = answer and plain and rows_per_group % bm == 0
        out["can_group"][shape] = dict(stages=stages, answer=answer)
    for nparts, groups, C, rows, dtype, sw in bn_shape_table(ops, B):
        switches({"VG_BN_FUSED_FWD": str(sw)})
        out["bn_fused"].append(dict(nparts=nparts, groups=groups, C=C, rows=rows, dtype=dtype, fused_fwd=sw,
                                    supported=bool(lib.vg_bn_finalize_act_forward_supported(nparts, groups, C, rows, dtype))))
    switches({})
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes:", len(out["cases"]), "cases,",
          sum(len(v) for v in out["networks"].values()), "network launches,", len(out["bn_fused"]), "BatchNorm shapes")


def add_rows() -> None:
    """Entries for the rows of ALL_CASES the fixture does not hold yet, from the plan query of the loaded library (see the
    module docstring); every recorded entry stays as it is."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from importlib import import_module
    import _gg_ref as R
    ops = import_module(PKG + ".ops")
    with open(OUT) as f:
        out = json.load(f)
    keys = list(next(iter(out["cases"].values()))["plan"])
    switch_names = sorted({n for c in R.ALL_CASES for n in c.switches})
    for c in R.ALL_CASES:
        if c.id in out["cases"]:
            continue
        for n in switch_names:
            os.environ.pop(n, None)
        os.environ.update(c.switches)
        ops.reload_switches()
        g = c.specs()[0]
        plan = ops.gather_gemm_plan(g, c.dtype, bias=c.has("b"), want_stats=c.has("s"), act=c.act, mask=c.mask)
        assert R.label(plan) == c.label, (c.id, R.label(plan))
        out["cases"][c.id] = dict(nparts=plan["nparts"], tile_m=plan["bm"], ws_bytes=plan["ws_bytes"], family=plan["timing_family"],
                                  tile_m_stats=ops.gather_gemm_plan(g, c.dtype, want_stats=True)["bm"],
                                  plan={k: list(plan[k]) if k == "detail" else plan[k] for k in keys})
        print("added", c.id, R.label(plan))
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    add_rows() if "--add-rows" in sys.argv[1:] else main()
