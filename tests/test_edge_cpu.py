"""CPU: the edge-layer restatements of tests/_edge_ref.py against torch in f64, the integer operands, the coverage of the two
launchers by the case tables of tests/test_gpu_edge.py -- read from the launchers' own plan records (vg_tnconv_plan and
vg_edge_wgrad_plan need no GPU), never from a copy of the planners -- and geometry.py's admission rules against the library's."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import _edge_ref as E
import _wgrad_ref as R
from _emulate import to_nhwc

G = R.G


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(R.PKG + ".ops")


def _close(actual, ref):
    # two f64 routes to the same sum: they differ by summation order only
    torch.testing.assert_close(actual, ref, rtol=1e-12, atol=1e-12)


# ---- the references against torch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,s", [(3, 1), (4, 2)])
@pytest.mark.parametrize("P", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_restated_transposed_conv_equals_torch(k, s, P, N):
    B, C, IH, IW = 2, 5, 6, 7                          # not square: a transposed index would show
    g = torch.Generator().manual_seed(100 * k + 10 * P + N)
    x = torch.randn(B, C, IH, IW, generator=g, dtype=torch.float64)
    w = torch.randn(C, N, k, k, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w, stride=s, padding=P)
    tn = G.TNSpec(B=B, IH=IH, IW=IW, C=C, N=N, K=k, S=s, P=P, OH=ref.shape[2], OW=ref.shape[3], OC=8, Wpitch=32)
    assert (tn.OH, tn.OW) == (G.convT_out(IH, k, s, P), G.convT_out(IW, k, s, P))
    _close(E.tnconv_ref(tn, to_nhwc(x, C), w), ref)


EW_REF_CASES = [  # H, C, N, k, s, p
    (8, 6, 3, 4, 2, 1), (9, 4, 2, 4, 2, 0), (8, 5, 1, 4, 2, 2), (7, 6, 3, 3, 1, 1), (6, 4, 2, 3, 1, 0), (7, 5, 1, 3, 1, 2),
    (9, 4, 3, 3, 2, 1), (6, 4, 2, 4, 1, 1),            # the two other (k, s) pairs vg_edge_wgrad admits
]


@pytest.mark.parametrize("H,C,N,k,s,p", EW_REF_CASES)
def test_restated_edge_weight_gradient_of_a_conv_equals_torch(H, C, N, k, s, p):
    B = 2
    g = torch.Generator().manual_seed(H * 100 + C)
    x = torch.randn(B, N, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(C, N, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    ref, = torch.autograd.grad(y, w, dy)
    ew = G.EWSpec(B=B, WH=y.shape[2], WW=y.shape[3], C=C, NH=H, NW=H, N=N, K=k, S=s, P=p, s_c=N * k * k, s_n=k * k)
    _close(E.edge_wgrad_ref(ew, to_nhwc(dy, C), to_nhwc(x, 8)).view(C, N, k, k), ref)


@pytest.mark.parametrize("H,C,N,k,s,p", EW_REF_CASES)
def test_restated_edge_weight_gradient_of_a_transposed_conv_equals_torch(H, C, N, k, s, p):
    B = 2
    g = torch.Generator().manual_seed(H * 100 + C + 1)
    x = torch.randn(B, C, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(C, N, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    ref, = torch.autograd.grad(y, w, dy)
    ew = G.EWSpec(B=B, WH=H, WW=H, C=C, NH=y.shape[2], NW=y.shape[3], N=N, K=k, S=s, P=p, s_c=N * k * k, s_n=k * k)
    _close(E.edge_wgrad_ref(ew, to_nhwc(x, C), to_nhwc(dy, 8)).view(C, N, k, k), ref)


def test_edge_spec_builders_agree_with_the_shapes_of_torch():
    """conv_wgrad_edge / convT_wgrad_edge (what the case table is built with) give the operand shapes and strides used above."""
    ew = G.conv_wgrad_edge(2, 64, 64, 2, 32, 4, 2, 0, G.BF16)
    assert (ew.WH, ew.WW, ew.C, ew.NH, ew.NW, ew.N, ew.s_c, ew.s_n) == (31, 31, 32, 64, 64, 2, 32, 16)
    ew = G.convT_wgrad_edge(2, 48, 48, 16, 2, 3, 1, 1, G.BF16)
    assert (ew.WH, ew.WW, ew.C, ew.NH, ew.NW, ew.N, ew.s_c, ew.s_n) == (48, 48, 16, 48, 48, 2, 18, 9)


# ---- the operands ------------------------------------------------------------------------------------------------------
def test_integer_operands_have_no_zero_in_a_real_channel_and_zero_padding():
    vals = {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    tn, _ = E.TN_CASES[0].spec()
    X, W = E.tn_operands(tn, 3)
    assert X.dtype == torch.bfloat16 and X.shape == (tn.B, tn.IH, tn.IW, tn.C) and W.shape == (tn.C, tn.N, tn.K, tn.K)
    assert set(X.float().flatten().tolist()) == vals and set(W.flatten().tolist()) == vals
    assert set(E.tn_eps(tn, 4).flatten().tolist()) == vals
    ew = E.EW_CASES[2].spec()
    wide, narrow = E.ew_operands(ew, 5)
    assert wide.shape == (ew.B, ew.WH, ew.WW, ew.C) and narrow.shape == (ew.B, ew.NH, ew.NW, 8) and ew.N == 2
    assert set(wide.float().flatten().tolist()) == vals and set(narrow[..., :2].float().flatten().tolist()) == vals
    assert (narrow[..., 2:] == 0).all()
    with pytest.raises(AssertionError):
        E.ew_operands(G.conv_wgrad_edge(64, 256, 256, 3, 16, 4, 2, 1, G.BF16), 0)      # 9 M leaves the exact range


def test_noise_scale_is_one_step_above_the_bf16_spacing():
    assert [E.bf16_spacing(x) for x in (1.0, 255.0, 256.0, 511.0, 5184.0)] == [2.0 ** -7, 1.0, 2.0, 4.0, 32.0]   # (511 rounds to 512)
    for top in (1.0, 127.0, 128.0, 300.0, 511.0, 5184.0):
        sigma = E.tn_sigma(torch.tensor([-top, 1.0]))
        assert sigma == 4 * E.bf16_spacing(2.0 ** torch.frexp(torch.tensor(top))[1].item() / 2)      # four steps at top's binade
        for v in (top, top + 3 * sigma, top - 3 * sigma):                                             # every reachable value:
            assert float(torch.tensor(v + sigma).to(torch.bfloat16)) != float(torch.tensor(v).to(torch.bfloat16))   # a unit shows


# ---- coverage: which kernels and tilings the tables reach, read from the plan records --------------------------------------
def test_transposed_conv_table_reaches_every_instantiation_and_tiling(ops, capsys):
    """Every row plans what it is listed with (without and, where listed, with in-kernel noise) and shows the facets it names;
    together the rows reach all 14 tnconv_kernel<nt, kc, ., K, S> and every facet of TN_FACETS."""
    reached, seen = set(), set()
    lines = []
    for case in E.TN_CASES:
        tn, _ = case.spec()
        p, r = ops.tnconv_plan(tn, rng=False), ops.tnconv_plan(tn, rng=True)
        lines.append(f"  {case.id:26s} {E.tn_plan_tuple(p)}  rng {E.tn_plan_tuple(r)}  {' '.join(case.why)}")
        assert E.tn_plan_tuple(p) == case.plan, (case.id, p)
        if case.rng_plan:
            assert E.tn_plan_tuple(r) == case.rng_plan, (case.id, r)
        assert any(f.startswith("rng_") for f in case.why) == bool(case.rng_plan), case.id
        for rec in (p, r):
            assert rec["npix"] == (512 if rec["nt"] <= 2 else 256) and rec["tc"] % 16 == 0 and rec["ro"] % tn.S == 0, (case.id, rec)
            assert rec["tiles_y"] == -(-tn.OH // rec["ro"]) and rec["tiles_x"] == -(-tn.OW // rec["co"]), (case.id, rec)
            assert rec["grid"] == tn.B * rec["tiles_x"] * rec["tiles_y"], (case.id, rec)
            assert ((rec["ro"] - 1 + tn.K - 1) // tn.S + 1) * rec["tc"] <= rec["npix"], (case.id, rec)   # the window fits the LDS tile
            assert (rec["tiles_x"] == 1) == (rec["tc"] == tn.IW and rec["co"] == tn.OW), (case.id, rec)   # whole rows <=> one column tile
        assert not p["quad_noise"] and r["quad_noise"] == (tn.OW % 4 == 0), case.id
        assert p["nt"] == -(-tn.K * tn.K * tn.N // 16) and p["kc"] == -(-tn.C // 32)
        reached.add((p["nt"], p["kc"], tn.K))
        reached.add((r["nt"], r["kc"], tn.K))
        for facet in case.why:
            assert E.TN_FACETS[facet](case, tn, p, r), f"{case.id} does not show '{facet}': {p} / rng {r}"
            seen.add(facet)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert reached == E.TN_INSTANTIATIONS, sorted(E.TN_INSTANTIATIONS - reached)
    assert seen == set(E.TN_FACETS), sorted(set(E.TN_FACETS) - seen)


def test_edge_weight_gradient_table_reaches_every_instantiation_and_walk(ops, capsys):
    """Every row plans what it is listed with and shows its facets; together: edge_wgrad_kernel<1 | 2 | 4> x 3 | 4 tap-row
    tiles, N = 1, 2, 3, short last tiles, and workgroups that walk 2 | 1 and 3 | 2 tiles (ntiles > grid)."""
    seen, lines, plans = set(), [], []
    for case in E.EW_CASES:
        ew = case.spec()
        p = ops.edge_wgrad_plan(ew)
        plans.append((ew, p))
        lines.append(f"  {case.id:34s} {E.ew_plan_tuple(p)} tiles/image {p['tiles_per_img']:3d} walk {E.ew_walk(p)}  {' '.join(case.why)}")
        assert E.ew_plan_tuple(p) == case.plan, (case.id, p)
        assert p["ct"] == ew.C // 16 and p["jt"] == (4 if ew.K == 4 else 3), (case.id, p)
        assert p["tiles_per_img"] == -(-ew.WH // p["rows_per_tile"]) and p["ntiles"] == ew.B * p["tiles_per_img"], (case.id, p)
        assert p["grid"] == min(p["ntiles"], 512) and p["ws_bytes"] == p["grid"] * p["jt"] * 16 * ew.C * 4, (case.id, p)
        assert p["rows_per_tile"] * ew.WW <= 256, (case.id, p)
        for facet in case.why:
            assert E.EW_FACETS[facet](ew, p), f"{case.id} does not show '{facet}': {p}"
            seen.add(facet)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert {(p["ct"], p["jt"]) for _, p in plans} == {(ct, jt) for ct in (1, 2, 4) for jt in (3, 4)}
    assert {ew.N for ew, _ in plans} == {1, 2, 3}
    assert seen == set(E.EW_FACETS), sorted(set(E.EW_FACETS) - seen)
    assert sum(p["ntiles"] > p["grid"] for _, p in plans) >= 4


def test_tolerance_table_of_the_edge_weight_gradient_has_no_walk(ops):
    """Every row of _wgrad_ref.EDGE_SHAPES (the tolerance test of tests/test_gpu_kernels.py) gives each workgroup ONE tile: the
    grid-stride walk is reached by the rows of _edge_ref.EW_CASES only."""
    for row in R.EDGE_SHAPES:
        p = ops.edge_wgrad_plan(R.edge_spec(*row))
        assert p["ntiles"] == p["grid"] < 512, (row, p)


# ---- geometry.py against the library ---------------------------------------------------------------------------------------
def test_every_edge_weight_gradient_geometry_admits_is_taken_by_the_library(ops):
    """edge_wgrad_spec applies the 22 KB patch limit to every C; the library allows 26 KB for C <= 32.  geometry.py may refuse
    what the library takes (the generic weight gradient runs then), never the reverse -- and at C = 64 the two agree."""
    L = importlib.import_module(R.PKG + "._lib")
    lib, wider = L.load(), []
    for k in (3, 4):
        for s in (1, 2):
            for C in (16, 32, 64):
                for ww in range(1, 257):
                    nw = (ww - 1) * s + k - 2
                    if nw <= 0:
                        continue
                    ew = G.EWSpec(B=2, WH=ww, WW=ww, C=C, NH=nw, NW=nw, N=3, K=k, S=s, P=1, s_c=3 * k * k, s_n=k * k)
                    admitted = G.edge_wgrad_spec(2, ww, ww, C, nw, nw, 3, k, s, 1, G.BF16, 3 * k * k, k * k)
                    assert admitted is None or admitted == ew
                    d, plan = ops._ew_desc(ew, True, True, True, True), L.EWPlan()
                    rc = lib.vg_edge_wgrad_plan(d, plan)
                    assert rc in (0, L.VG_ENOSUP), (ew, rc)
                    if admitted is not None:
                        assert rc == 0, f"geometry.py admits {ew}, the library answers {rc}"
                    elif rc == 0:
                        wider.append((k, s, C, ww))
    assert wider and all(C <= 32 for _, _, C, _ in wider), wider[:5]
    assert {s for _, s, _, _ in wider} == {2} and min(w for _, _, _, w in wider) > 128, wider[:5]   # stride 2 onto maps wider than any member's


def test_every_transposed_conv_geometry_admits_is_taken_by_the_library(ops):
    refused = []
    for k, s in ((3, 1), (4, 2)):
        for P in (0, 1, 2):
            for N in (1, 2, 3, 4):
                for C in (16, 32, 64):
                    for iw in range(16, 513, 16):
                        sp = G.tn_spec(2, iw, iw, C, N, k, s, P, G.BF16, k * k, N * k * k)
                        if sp is None:
                            continue
                        for rng in (False, True):
                            try:
                                p = ops.tnconv_plan(sp[0], rng=rng)
                            except RuntimeError as e:
                                refused.append((k, s, P, N, C, iw, rng, str(e)))
                                continue
                            # what keeps the kernel inside its LDS tile: the rows and the columns behind an output tile fit
                            assert ((p["ro"] - 1 + k - 1) // s + 1) * p["tc"] <= p["npix"], (k, s, P, N, C, iw, rng, p)
                            assert p["tc"] == iw or (p["co"] - 1 + k - 1) // s + 1 <= p["tc"], (k, s, P, N, C, iw, rng, p)
    assert not refused, refused[:5]
    assert G.tn_spec(2, 512, 512, 16, 4, 4, 2, 2, G.BF16, 16, 64) is not None           # the sweep's corner is admitted
