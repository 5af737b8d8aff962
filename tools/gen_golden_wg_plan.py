"""Writes tests/golden/wg_plan_parent.json: what the weight-gradient size queries vg_wgrad_ws_bytes / vg_edge_wgrad_ws_bytes
answered, and what the Python restatement of the launcher (tests/_wgrad_ref.plan) derived from the answer, per geometry,
BEFORE vg_wgrad / vg_edge_wgrad were moved onto the plan records vg_wg_plan / vg_ew_plan (ABI 23 deleted both size queries
and plan()).  tests/test_wgrad_cpu.py asserts that the records reproduce all of it.

It was run ONCE, at commit d3a4b7d ("Keep loads in flight: BatchNorm slab sums, streaming narrow-K conv", ABI 22), on the
built library, host only (no GPU), with the one new row of the case table (XCD_DEFAULT) already in tests/_wgrad_ref.py:

    python tools/gen_golden_wg_plan.py

It CANNOT be re-run on a later checkout: the exports and the function it records are gone.  It stays as the record of how
the fixture was made:

  ws_bytes      vg_wgrad_ws_bytes asked as ops.wgrad asked it: geometry and a non-NULL `zeros` (the zero page), nothing else
  the rest      _wgrad_ref.plan(spec, dtype, ws_bytes, <the switch values of the row>): nsplit, rows_per_split, last_rows,
                partial_stage, main, reduce
  edge rows     vg_edge_wgrad_ws_bytes of the geometry

Rows: "cases" -- every (case, dtype) of _wgrad_ref.CASE_PARAMS under its own switches; "switches" -- every row of
SWITCH_PARAMS; "networks" -- under the default switches every weight gradient of the three networks at the benchmarked
shapes (_wgrad_ref.network_wgrads); "edge" -- the shape list of the edge-layer GPU test (_wgrad_ref.EDGE_SHAPES).

tests/test_wgrad_cpu.py used to ask with zeros = NULL, which the launcher reads as "register-staged kernel", and label the
answer as the LDS-DMA kernels.  The generator asserts for every row that the two answers were equal at the parent (the
stage rows of the two kernels happened to agree), so that test's history is not a different record.
"""
import json
import os
import sys
from ctypes import byref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "wg_plan_parent.json")
SOME = 64                                   # non-NULL, 16-byte aligned; the queries never dereference a pointer


def main() -> None:
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from importlib import import_module
    import _gg_ref
    import _wgrad_ref as R
    L, ops = import_module(R.PKG + "._lib"), import_module(R.PKG + ".ops")
    lib = L.load()
    assert lib.vg_abi_version() == 22, "the size queries exist up to ABI 22 only"
    switch_names = sorted({n for n, _ in R.SWITCHES})

    def switches(env):
        for n in switch_names:
            os.environ.pop(n, None)
        os.environ.update({n: str(v) for n, v in env.items()})
        ops.reload_switches()

    def wg_row(wg, dtype, sw):
        def ask(zeros):
            d = L.WGDesc(B=wg.B, GH=wg.GH, GW=wg.GW, PC=wg.PC, NP=wg.NP, QH=wg.QH, QW=wg.QW, QC=wg.QC, NQ=wg.NQ, SY=wg.SY,
                         SX=wg.SX, DY=wg.DY, DX=wg.DX, TH=wg.TH, TW=wg.TW, y0=wg.y0, x0=wg.x0, s_np=wg.s_np, s_cq=wg.s_cq,
                         s_t=wg.s_t, zeros=zeros)
            n = lib.vg_wgrad_ws_bytes(byref(d), dtype)
            assert n > 0, n
            return int(n)
        ws_bytes = ask(SOME)
        assert ask(0) == ws_bytes, "zeros = NULL sized another workspace than the zero page"
        p = R.plan(wg, dtype, ws_bytes, wg_spec=sw.get("VG_WG_SPEC", 3), wg_dma=sw.get("VG_WG_DMA", 1),
                   wg_reduce_t=sw.get("VG_WG_REDUCE_T", 1))
        return dict(ws_bytes=ws_bytes, **{k: p[k] for k in ("nsplit", "rows_per_split", "last_rows", "partial_stage", "main",
                                                            "reduce")})

    def ew_row(ew):
        d = L.EWDesc(B=ew.B, WH=ew.WH, WW=ew.WW, C=ew.C, NH=ew.NH, NW=ew.NW, N=ew.N, K=ew.K, S=ew.S, P=ew.P, s_c=ew.s_c,
                     s_n=ew.s_n)
        n = lib.vg_edge_wgrad_ws_bytes(byref(d))
        assert n > 0, n
        return dict(ws_bytes=int(n))

    out = dict(parent="d3a4b7d", cases={}, switches={}, networks={}, edge={})
    for (case, dtype), cid in zip(R.CASE_PARAMS, R.CASE_IDS):
        sw = {"VG_WG_TARGET": case.target} if case.target else {}
        switches(sw)
        out["cases"][cid] = wg_row(case.spec(dtype), dtype, sw)
    for (case, dtype, name, val), sid in zip(R.SWITCH_PARAMS, R.SWITCH_IDS):
        switches({name: val})
        out["switches"][sid] = wg_row(case.spec(dtype), dtype, {name: val})
    switches({})
    for S, nb, dtype in _gg_ref.NETWORK_SHAPES:
        out["networks"][f"S{S}_B{nb}_{dtype}"] = {key: ew_row(sp) if kdt is None else wg_row(sp, kdt, {})
                                                 for key, sp, kdt in R.network_wgrads(S, nb, dtype)}
    for row in R.EDGE_SHAPES:
        out["edge"][R.edge_id(*row)] = ew_row(R.edge_spec(*row))
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes:", len(out["cases"]), "cases,", len(out["switches"]), "switch rows,",
          sum(len(v) for v in out["networks"].values()), "network weight gradients,", len(out["edge"]), "edge shapes")


if __name__ == "__main__":
    main()
