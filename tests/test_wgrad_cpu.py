"""CPU: the weight-gradient restatement of tests/_wgrad_ref.py against torch in f64 (which also validates the WGSpec
builders of geometry.py), the blind-spot check of the integer case table, and the coverage of the launcher's branches by
that table, read from the launcher's own plan record (vg_wgrad_plan / vg_edge_wgrad_plan need no GPU) and held against what
the parent commit planned (tests/golden/wg_plan_parent.json, tools/gen_golden_wg_plan.py)."""
import dataclasses
import importlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

import _wgrad_ref as R
from _emulate import to_nhwc

G = R.G
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wg_plan_parent.json")) as _f:
    PARENT = json.load(_f)

REF_CASES = [  # B, H, Cin, Cout, k, s, p
    (2, 8, 8, 16, 4, 2, 1),          # k4 s2 p1
    (2, 9, 8, 8, 4, 2, 0),           # k4 s2 p0, odd H: the last row and column lie outside every window
    (3, 7, 8, 8, 3, 1, 1),           # k3 s1 p1
    (2, 8, 6, 10, 4, 2, 1),          # channel counts that are no multiple of 8 (nor of 4): padded operands
    (2, 5, 3, 12, 3, 1, 1),
]


def _close(actual, ref):
    # two f64 routes to the same sum: they differ by summation order only
    torch.testing.assert_close(actual, ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", REF_CASES)
def test_restated_conv_weight_gradient_equals_torch(dtype, B, H, Cin, Cout, k, s, p):
    g = torch.Generator().manual_seed(H * 100 + Cin)
    x = torch.randn(B, Cin, H, H, generator=g, dtype=torch.float64)
    OH = G.conv_out(H, k, s, p)
    dy = torch.randn(B, Cout, OH, OH, generator=g, dtype=torch.float64)
    ref = torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), dy, stride=s, padding=p)
    wg = G.conv_wgrad(B, H, H, Cin, Cout, k, s, p, dtype)
    got = R.wgrad_ref(wg, to_nhwc(dy, wg.PC), to_nhwc(x, wg.QC))
    _close(got.view(Cout, Cin, k, k), ref)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,Cin,Cout,k,s,p", REF_CASES)
def test_restated_transposed_conv_weight_gradient_equals_torch(dtype, B, H, Cin, Cout, k, s, p):
    g = torch.Generator().manual_seed(H * 100 + Cin + 1)
    x = torch.randn(B, Cin, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(Cin, Cout, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, None, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    ref, = torch.autograd.grad(y, w, dy)
    wg = G.convT_wgrad(B, H, H, Cin, Cout, k, s, p, dtype)
    got = R.wgrad_ref(wg, to_nhwc(x, wg.PC), to_nhwc(dy, wg.QC))
    _close(got.view(Cin, Cout, k, k), ref)


@pytest.mark.parametrize("dtype", [G.F32, G.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,H,C,N", [(5, 2, 8, 12), (4, 1, 16, 6), (3, 6, 6, 10), (7, 3, 3, 5)])
def test_restated_linear_weight_gradient_equals_torch(dtype, B, H, C, N):
    g = torch.Generator().manual_seed(H * 100 + C + 2)
    h = torch.randn(B, C, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(N, C * H * H, dtype=torch.float64, requires_grad=True)
    out = F.linear(h.flatten(1), w)                       # nn.Linear on the NCHW-flattened map
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    ref, = torch.autograd.grad(out, w, dout)
    wg = G.linear_wgrad(B, H, H, C, N, dtype)
    got = R.wgrad_ref(wg, to_nhwc(dout.view(B, N, 1, 1), wg.PC), to_nhwc(h, wg.QC))
    _close(got.view(N, C * H * H), ref)


def test_integer_operands_have_no_zero_in_a_real_channel_and_zero_padding():
    wg = G.conv_wgrad(3, 8, 8, 6, 10, 4, 2, 1, G.BF16)
    P, Q = R.int_operands(wg, G.BF16, 5)
    assert P.dtype == torch.bfloat16 and P.shape == (3, 4, 4, 16) and Q.shape == (3, 8, 8, 8)
    for t, real in ((P, 10), (Q, 6)):
        assert set(t[..., :real].float().flatten().tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
        assert (t[..., real:] == 0).all()
    with pytest.raises(AssertionError):
        R.int_operands(G.conv_wgrad(64, 256, 256, 8, 8, 4, 2, 1, G.F32), G.F32, 0)     # 9 M leaves the exact range


@pytest.mark.parametrize("case,dtype", R.CASE_PARAMS, ids=R.CASE_IDS)
def test_every_case_reads_the_element_that_is_negated(case, dtype):
    """Blind spots: negating one randomly chosen real element of P, and separately of Q, must change the reference result.
    The reference is linear in each operand and a sum over images, so the change is the reference of (the difference,
    the other operand) of that one image: exact in integers, and it must not be zero."""
    wg = case.spec(dtype)
    P, Q = R.int_operands(wg, dtype, 1)
    one = dataclasses.replace(wg, B=1)
    g = torch.Generator().manual_seed(17)

    def pick(*dims):
        return tuple(int(torch.randint(0, d, (1,), generator=g)) for d in dims)

    b, gy, gx, ch = pick(wg.B, wg.GH, wg.GW, wg.NP)
    dP = torch.zeros_like(P[b:b + 1])
    dP[0, gy, gx, ch] = -2 * P[b, gy, gx, ch]
    assert R.wgrad_ref(one, dP, Q[b:b + 1]).abs().max() > 0, ("P", b, gy, gx, ch)
    b, iy, ix, ch = pick(wg.B, wg.QH, wg.QW, wg.NQ)
    dQ = torch.zeros_like(Q[b:b + 1])
    dQ[0, iy, ix, ch] = -2 * Q[b, iy, ix, ch]
    assert R.wgrad_ref(one, P[b:b + 1], dQ).abs().max() > 0, ("Q", b, iy, ix, ch)


def _same_as_parent(p, want, what):
    """p: R.facts of the launcher's record; want: the fixture row of the same geometry and switches."""
    for key in ("ws_bytes", "nsplit", "rows_per_split", "last_rows", "partial_stage", "main", "reduce"):
        assert p[key] == want[key], f"{what}: {key} is {p[key]}, the parent commit planned {want[key]}"


def test_case_table_reaches_every_branch_of_the_launcher(vg_switch, monkeypatch, capsys):
    """The launcher's own record (ops.wgrad_plan), over the case table and the switch settings of tests/test_gpu_wgrad.py:
    every row reaches the kernels it is labelled with and plans what the parent commit planned, and the labels name every
    main kernel and every reduce-kernel form vg_wgrad can launch."""
    ops = importlib.import_module(R.PKG + ".ops")
    names = sorted({n for n, _ in R.SWITCHES})
    rows = []

    def record(name, want, case, dtype, **sw):
        for n in names:
            monkeypatch.delenv(n, raising=False)
        ops.reload_switches()
        for n, v in sw.items():
            vg_switch(n, v)
        wg = case.spec(dtype)
        p = R.facts(wg, ops.wgrad_plan(wg, dtype))
        _same_as_parent(p, want, name)
        rows.append((name, sw, dtype, p))

    for (case, dtype), name in zip(R.CASE_PARAMS, R.CASE_IDS):
        record(name, PARENT["cases"][name], case, dtype, **({"VG_WG_TARGET": case.target} if case.target else {}))
        assert (rows[-1][3]["main"], rows[-1][3]["reduce"]) == case.kernels(dtype), name
        assert rows[-1][3]["xcd_order"] == (case is R.XCD_DEFAULT), name
    n_table = len(rows)
    for (case, dtype, sw_name, val), sid in zip(R.SWITCH_PARAMS, R.SWITCH_IDS):
        record(f"{case.id}-{R.DT_NAME[dtype]}", PARENT["switches"][sid], case, dtype, **{sw_name: val})
        assert rows[-1][3]["xcd_order"] == (sw_name == "VG_WG_XCD"), sid             # =2: always; no other row qualifies
    with capsys.disabled():
        for name, sw, _, p in rows:
            print(f"\n  {name:42s} {str(sw or ''):26s} nsplit {p['nsplit']:3d} rows/split {p['rows_per_split']:5d} "
                  f"last {p['last_rows']:5d}  {p['main']:8s} {p['reduce']}{' xcd' if p['xcd_order'] else ''}", end="")
        print()

    table = [p for _, _, _, p in rows[:n_table]]
    rt = [p for p in table if p["reduce"] == "reduce_t"]
    for lo, hi in ((1, 1), (2, 3), (5, 7), (9, 16)):
        assert any(lo <= p["nsplit"] <= hi for p in rt), f"no reduce_t case with nsplit in [{lo}, {hi}]"
    for T in (16, 9, 4, 1):
        assert any(p["T"] == T for p in rt), f"no reduce_t case with {T} taps"
    have = {p["reduce"] for p in table}
    for label in ("generic<4,4> SPL=1", "generic<4,4> SPL=8", "generic<4,4> SPL=32", "generic<4,1> SPL=8"):
        assert label in have, label
    assert any(r.startswith("generic<16,4>") for r in have) and any(r.startswith("generic<16,1>") for r in have), have
    bf16_main = {p["main"] for (_, _, dt, p) in rows[:n_table] if dt == G.BF16}
    assert {"ws<1,8>", "ws<2,8>"} <= bf16_main, bf16_main
    assert any(p["partial_stage"] and p["nsplit"] > 1 for p in table), "no case whose last split holds a partial stage"
    assert any(p["main"] == "f32" for p in table)
    # the switch settings add the three non-default main kernels and move cases between the reduce kernels and split counts
    switched = rows[n_table:]
    assert {"bf16_dma", "bf16_reg", "ws<2,4>", "ws<1,8>"} <= {p["main"] for _, _, _, p in switched}
    base = {name: p for name, _, _, p in rows[:n_table]}
    assert any(sw == {"VG_WG_REDUCE_T": 0} and base[name]["reduce"] == "reduce_t" and p["reduce"].startswith("generic")
               for name, sw, _, p in switched)
    # (every case of the subset is already limited by its stage count at the default target: 4096 repeats the default split)
    assert any(sw == {"VG_WG_TARGET": 64} and p["nsplit"] != base[name]["nsplit"] for name, sw, _, p in switched)


def test_networks_plan_what_the_parent_commit_planned(monkeypatch):
    """Under the default switches, every weight gradient of the three networks at the benchmarked shapes: the records of
    vg_wgrad_plan / vg_edge_wgrad_plan against the workspace sizes and kernels of the parent commit."""
    import _gg_ref
    ops = importlib.import_module(R.PKG + ".ops")
    for n in {n for n, _ in R.SWITCHES}:
        monkeypatch.delenv(n, raising=False)
    ops.reload_switches()
    for S, nb, dtype in _gg_ref.NETWORK_SHAPES:
        want = PARENT["networks"][f"S{S}_B{nb}_{dtype}"]
        launches = R.network_wgrads(S, nb, dtype)
        assert sorted(key for key, _, _ in launches) == sorted(want)
        for key, sp, kdt in launches:
            if kdt is None:
                assert ops.edge_wgrad_plan(sp)["ws_bytes"] == want[key]["ws_bytes"], key
            else:
                _same_as_parent(R.facts(sp, ops.wgrad_plan(sp, kdt)), want[key], f"S{S} B{nb} {dtype} {key}")


def test_edge_shapes_reach_every_instantiation_of_the_edge_kernel():
    """The shape list of the edge-layer GPU test (tests/test_gpu_kernels.py), asked of vg_edge_wgrad_plan: it reaches
    edge_wgrad_kernel<1 | 2 | 4> with 3 and 4 tap-row tiles, and sizes the workspace as the parent commit did."""
    ops = importlib.import_module(R.PKG + ".ops")
    plans = {}
    for row in R.EDGE_SHAPES:
        ew = R.edge_spec(*row)
        assert ew is not None, row
        p = plans[R.edge_id(*row)] = ops.edge_wgrad_plan(ew)
        assert p["ws_bytes"] == PARENT["edge"][R.edge_id(*row)]["ws_bytes"], row
        assert p["ct"] == ew.C // 16 and p["jt"] == (4 if ew.K == 4 else 3), (row, p)
        assert p["tiles_per_img"] == -(-ew.WH // p["rows_per_tile"]) and p["ntiles"] == ew.B * p["tiles_per_img"], (row, p)
        assert p["grid"] == min(p["ntiles"], 512) and p["ws_bytes"] == p["grid"] * p["jt"] * 16 * ew.C * 4, (row, p)
    assert {p["ct"] for p in plans.values()} == {1, 2, 4} and {p["jt"] for p in plans.values()} == {3, 4}
