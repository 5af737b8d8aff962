"""CPU: the gather-GEMM case table of tests/_gg_ref.py before it meets a kernel.

  * every geometry builder (G.*_fprop / G.*_dgrad) and the packer's layout, restated at descriptor level by
    tests/_emulate.py, against torch's own convolutions in f64 on the table's integer operands -- exactly;
  * the descriptor-level statistics slabs and written mask against the vectorised ones the GPU test uses;
  * the exactness conditions (every sum below 2^24), the operand generator, the blind spots of every row;
  * the coverage of the launcher's branches by the table, read from the built library (vg_gather_gemm_plan needs no GPU);
  * the plan record against the side queries it replaced (tests/golden/gg_plan_parent.json), for the table and for every
    launch of the three networks at the benchmarked shapes, and the placeholder workspace of ops.gather_gemm.

No tolerance anywhere: integer operands make every comparison an equality."""
import dataclasses
import functools
import importlib
import json
import os

import pytest
import torch

import _gg_ref as R
from _emulate import emulate_gg, emulate_pack

G = R.G
SWITCH_NAMES = sorted({n for c in R.ALL_CASES for n in c.switches})


@pytest.fixture
def set_case_switches(vg_switch, monkeypatch):
    """The switches of one table row (vg_switch restores and re-reads the defaults when the test ends)."""
    ops = importlib.import_module(R.PKG + ".ops")

    def apply(case):
        for n in SWITCH_NAMES:
            monkeypatch.delenv(n, raising=False)
        for n, v in case.switches.items():
            monkeypatch.setenv(n, v)
        ops.reload_switches()
        return ops.gather_gemm_plan(case.specs()[0], case.dtype, bias=case.has("b"), want_stats=case.has("s"), act=case.act,
                                    mask=case.mask)

    return apply


@functools.lru_cache(maxsize=None)
def _problem(case):
    ops_ = R.operands(case)
    return ops_, R.preact_ref(case, ops_)


# ---- builders and packer against torch ------------------------------------------------------------------------------------
def _small(case):
    g, pk = case.specs()
    return g.nphase * g.GH * g.GW * g.TH * g.TW <= 2500 and pk.nphase * pk.TH * pk.TW * pk.C <= 3000


SMALL = [c for c in R.CASES if _small(c)]


def test_the_small_members_cover_every_builder():
    kinds = {c.kind for c in SMALL}
    assert kinds == {"conv", "convT", "conv_dgrad", "convT_dgrad", "linear", "linear_dgrad"}, kinds
    forms = {(c.kind, c.specs()[0].nphase, c.specs()[1].tap_in_n) for c in SMALL}
    assert ("convT", 4, 0) in forms and ("convT", 1, 0) in forms and ("convT", 1, 1) in forms      # 4-phase, stride 1, 1 x 1 input
    assert ("conv_dgrad", 4, 0) in forms and ("conv_dgrad", 1, 0) in forms
    assert any(R.skipped_pairs(c.specs()[0]) for c in SMALL)


def _slabs_by_definition(g, Y, bm):
    """The header's sentence, one (phase, grid pixel) at a time."""
    M = g.B * g.GH * g.GW
    mt = -(-M // bm)
    out = torch.zeros(g.nphase * mt, 2, g.N, dtype=torch.float64)
    for p in range(g.nphase):
        for b in range(g.B):
            for gy in range(g.GH):
                for gx in range(g.GW):
                    oy, ox = gy * g.OSY + g.ooy[p], gx * g.OSX + g.oox[p]
                    if oy < g.OH and ox < g.OW:
                        m = (b * g.GH + gy) * g.GW + gx
                        out[p * mt + m // bm, 0] += Y[b, oy, ox, :g.N]
                        out[p * mt + m // bm, 1] += Y[b, oy, ox, :g.N] ** 2
    return out


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_descriptor_and_pack_layout_of_every_builder_equal_torch(case):
    """emulate_pack + emulate_gg walk the PackSpec and the GGSpec index by index as include/vaegan_hip.h states them; on the
    integer operands their f64 result has to BE torch's (both are exact).  Then the written mask and the statistics slabs
    the GPU test derives from the descriptor in vectorised form, against the same walk."""
    g, pk = case.specs()
    ops_, yf = _problem(case)
    Wp = emulate_pack(pk, ops_["w"])
    Y, written = emulate_gg(g, R.x_nhwc(case, ops_["x"]).double(), Wp, ops_["bias"])
    assert torch.equal(Y[..., :g.N], yf)
    assert (Y[..., g.N:] == 0).all()
    assert torch.equal(written, R.written_mask(g))
    for bm in (64, 256):
        assert torch.equal(R.stats_ref(g, yf, bm), _slabs_by_definition(g, Y, bm))


def test_every_builder_writes_every_output_pixel_once_and_odd_maps_skip_grid_pixels():
    """Which descriptors skip output pixels: the 4-phase transposed form of an ODD map (data gradient of a stride-2 Conv2d
    whose input side is odd) has grid pixels beyond the last row / column in three of its phases.  No builder leaves an
    output pixel unwritten or writes one twice, so the GPU test compares whole tensors."""
    skipping = set()
    for c in R.ALL_CASES:
        g, _ = c.specs()
        assert (R.written_mask(g) == 1).all(), c.id
        if R.skipped_pairs(g):
            skipping.add((c.kind, g.nphase))
            assert g.OH % 2 == 1 and g.GH * 2 == g.OH + 1
    assert skipping == {("conv_dgrad", 4)}


# ---- operands -------------------------------------------------------------------------------------------------------------
def test_operands_hold_only_the_stated_values_and_zero_padding():
    for case, vals, padded in ((R.GENERIC[11], {1, 2, 3}, True), (R.FP8[2], {1}, False)):
        g, _ = case.specs()
        o = R.operands(case)
        want = {float(s * v) for v in vals for s in (-1, 1)}
        assert set(o["x"].flatten().tolist()) == want and set(o["w"].flatten().tolist()) == want
        X = R.x_nhwc(case, o["x"])
        C = case.x_shape()[1]
        assert X.shape == (g.B, g.IH, g.IW, g.IC) and (g.IC > C) == padded
        assert (X[..., C:] == 0).all() and (X[..., :C] != 0).all()
        assert set(X.double().flatten().tolist()) == want | ({0.0} if padded else set())    # exact in the storage dtype
    o = R.operands(R.GENERIC[1])                                                       # 'mr' on the f32 128 x 128 tile
    assert set(o["mask"].flatten().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    o = R.operands(R.GENERIC[0])
    assert o["bias"].abs().max() <= 4 and (o["bias"] == o["bias"].round()).all() and o["mask"] is None
    assert R.ACT_SLOPE == 0.25 and R.MASK_SLOPE == 0.5
    with pytest.raises(AssertionError):
        R.operands(dataclasses.replace(R.FP8[0], vals=3))


def test_output_reference_rounds_to_nearest_even_and_masks_on_the_boundary():
    case = dataclasses.replace(R.GENERIC[11], B=1, H=1, Cout=3)                        # bf16, LeakyReLU
    y = torch.tensor([257.0, 259.0, -1026.0]).view(1, 1, 1, 3)                          # bf16 keeps 8 bits: ties go to even
    Y = R.output_ref(case, dict(mask=None), y)
    assert Y.dtype == torch.bfloat16 and Y.shape[-1] == 8
    assert Y[0, 0, 0].tolist() == [256.0, 260.0, -256.0, 0, 0, 0, 0, 0]                 # -1026 / 4 = -256.5 -> -256
    case = dataclasses.replace(case, epi="mr")
    m = torch.tensor([1.0, 0.0, -1.0] + [1.0] * 5).view(1, 1, 1, 8)
    assert R.output_ref(case, dict(mask=m), y)[0, 0, 0].tolist() == [256.0, 0, 0, 0, 0, 0, 0, 0]     # a zero mask is NOT '> 0'


# ---- every row: exactness conditions and blind spots ------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.ALL_IDS)
def test_every_sum_of_the_case_is_exact_in_f32(case, set_case_switches):
    plan = set_case_switches(case)
    ops_, yf = _problem(case)
    assert R.exactness(case, ops_, yf, plan["bm"]) == []
    assert float(yf.abs().max()) < R.EXACT


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.ALL_IDS)
def test_every_case_reads_the_element_that_is_negated(case, set_case_switches):
    """Blind spots: negating one randomly chosen element of the gathered tensor, and separately one weight, must change the
    reference output (the map is linear in each: the change is the map of the difference, exact in integers) -- and, where
    the case has statistics, its slabs."""
    plan = set_case_switches(case)
    g, _ = case.specs()
    ops_, yf = _problem(case)
    x, w = ops_["x"], ops_["w"]
    gen = torch.Generator().manual_seed(17)

    def pick(shape):
        return tuple(int(torch.randint(0, d, (1,), generator=gen)) for d in shape)

    i = pick(x.shape)
    one = dataclasses.replace(case, B=1)
    dx = torch.zeros_like(x[:1])
    dx[(0,) + i[1:]] = -2 * x[i]
    dy = torch.zeros_like(yf)
    dy[i[0]:i[0] + 1] = R.to_output_layout(dataclasses.replace(g, B=1), R.core(one, dx, w))
    j = pick(w.shape)
    dw = torch.zeros_like(w)
    dw[j] = -2 * w[j]
    for what, d in (("x", dy), ("w", R.to_output_layout(g, R.core(case, x, dw)))):
        assert d.abs().max() > 0, (what, i, j)
        if case.has("s"):
            assert not torch.equal(R.stats_ref(g, yf + d, plan["bm"]), R.stats_ref(g, yf, plan["bm"])), (what, i, j)


# ---- coverage: what the library says it launches ----------------------------------------------------------------------------
def test_case_table_reaches_every_branch_of_the_launcher(set_case_switches, capsys):
    rows = [(c, set_case_switches(c)) for c in R.ALL_CASES]
    with capsys.disabled():
        for c, p in rows:
            split = f"ksplit {p['ksplit']:2d} x {p['stages_per_split']} of {p['nstages']}" if p["ksplit"] > 1 else ""
            print(f"\n  {c.id:66s} {R.label(p):28s} {split:20s} {'n-major ' if p['n_major'] else ''}"
                  f"{'slabs ' + str(p['nparts']) if p['nparts'] else ''}", end="")
        print()
    for c, p in rows:                                                  # a row whose plan is not the branch it names fails
        assert R.label(p) == c.label, (c.id, R.label(p), p)
        g, _ = c.specs()
        assert p["nparts"] == (g.nphase * -(-g.M // p["bm"]) if c.has("s") else 0), c.id
    table = rows[:len(R.CASES)]
    have = {(c.dtype, R.label(p)) for c, p in table}
    tiles = ("64x64", "128x64", "128x128", "128x32", "256x16")
    for t in tiles:                                                    # generic tiles: f32; bf16 on the ring and register-staged
        assert (G.F32, f"gg {t} reg") in have, t
        assert (G.BF16, f"gg {t} reg") in have, t
    for t in tiles[:3]:
        assert (G.BF16, f"gg {t} dma") in have, t
        assert (G.FP8, f"gg {t} dma") in have and (G.FP8, f"gg {t} reg") in have, t
    for lab in ("ggn<1,3>", "ggn<1,4>", "ggn<4,3>", "ggn<4,4>", "ggq<16,7>", "ggq<32,7>", "ggq<16,9>", "ggq<32,9>",
                "ggp<2>", "ggp<4>", "ggp<4,64>", "ggp<2,64>", "ggp<2,64,3>", "ggp<2,32>"):
        assert (G.BF16, lab) in have, lab

    def family(c, p):
        return "fp8" if c.dtype == G.FP8 else p["family"] + ("-split" if p["ksplit"] > 1 else "")

    # ragged / padded shapes on every generic tile: M and N no multiples of the tile, OC > N, a partial last stage
    for dt in (G.F32, G.BF16):
        for t in tiles:
            bm, bn = (int(v) for v in t.split("x"))
            assert any(c.dtype == dt and p["family"] == "generic" and (p["bm"], p["bn"]) == (bm, bn) and c.specs()[0].M % bm
                       and c.specs()[0].N % bn and c.specs()[0].OC > c.specs()[0].N and
                       (dt == G.F32 or p["nstages"] * (4 if p["dma"] and bm == 64 else 2) > c.specs()[0].Kp // 32)
                       for c, p in table), (dt, t)
    # epilogues: each on every family that accepts it (validate: no activation with statistics; narrowk_ok: no mask;
    # plan_splitk: bias and statistics only; fp8: no mask)
    accepts = {"generic": "b s r l mr ml", "narrowk": "b s r l", "phase4": "b s r l mr ml", "patch": "b s r l mr ml",
               "generic-split": "b s", "fp8": "b s r l"}
    for fam, epis in accepts.items():
        for e in epis.split():
            assert any(family(c, p) == fam and c.has(e) for c, p in table), (fam, e)
    # narrow-K: a last workgroup that is not full; stride 2 with padding 0 and with padding 1
    nk = [c for c, p in table if p["family"] == "narrowk"]
    assert all(c.specs()[0].M % 256 for c in nk) and {(c.s, c.p) for c in nk} >= {(2, 0), (2, 1), (1, 1)}
    # four-phase: 16 x 16 / 8 x 8 / 4 x 4 / 128-wide grids, 12 and 24 real columns
    q4 = [c.specs()[0] for c, p in table if p["family"] == "phase4"]
    assert {g.GW for g in q4} >= {4, 8, 16, 128} and {g.N for g in q4} >= {12, 24}
    # patch: both forms, several images per tile and a tile that is part of one image, on the 128- and the 256-row kernels
    pt = [(c.specs()[0], p) for c, p in table if p["family"] == "patch"]
    for bm in (128, 256):
        assert any(g.nphase == 4 and p["bm"] == bm for g, p in pt) and any(g.TH == 4 and p["bm"] == bm for g, p in pt)
        assert any(g.GH * g.GW < bm and p["bm"] == bm for g, p in pt) and any(g.GH * g.GW > bm and p["bm"] == bm for g, p in pt)
    # split K: flat on both main kernels with ksplit < 8 and > 8 (no multiple of 8), a shorter last slice; the tile reduce with
    # phases, statistics, a bias and OC > N; the big-K form
    sp = [(c, p) for c, p in table if p["ksplit"] > 1]
    for dma in (True, False):
        flat = [(c, p) for c, p in sp if p["reduce"] == "flat" and p["dma"] == dma and c.dtype == G.BF16]
        assert any(p["ksplit"] < 8 for _, p in flat) and any(p["ksplit"] > 8 and p["ksplit"] % 8 for _, p in flat), dma
        assert any(0 < p["nstages"] - (p["ksplit"] - 1) * p["stages_per_split"] < p["stages_per_split"] for _, p in flat), dma
    assert any(c.dtype == G.F32 and p["ksplit"] >= 16 for c, p in sp)
    tile = [(c, c.specs()[0], p) for c, p in sp if p["reduce"] == "tile"]
    assert any(g.nphase == 4 and c.has("s") and c.has("b") and g.OC > g.N for c, g, p in tile)
    assert any(g.nphase == 4 and not c.has("s") for c, g, p in tile) and any(g.nphase == 1 and c.has("s") for c, g, p in tile)
    assert {p["dma"] for _, _, p in tile} == {True, False}
    assert any((g.M, g.N, g.Kp, p["bm"], p["bn"], p["dma"]) == (1024, 1024, 2048, 128, 128, True) and p["ksplit"] * 64 >= 512
               for c, g, p in [(c, c.specs()[0], p) for c, p in sp])
    # fp8: one case with phases, one with statistics
    assert any(c.dtype == G.FP8 and c.specs()[0].nphase == 4 for c, _ in table)
    assert any(c.dtype == G.FP8 and c.has("s") for c, _ in table)
    # VG_GG_NMAJOR: =2 turns the order on exactly where the n-tile count is a multiple of 8, =0 turns it off everywhere
    switched = rows[len(R.CASES):]
    for c, p in switched:
        mode = c.switches["VG_GG_NMAJOR"]
        assert p["n_major"] == (mode == "2" and c.id in R.NMAJOR_TILES8), (c.id, p)
    assert {p["family"] for c, p in switched if p["n_major"]} == {"generic", "patch"}
    assert any(p["n_major"] for c, p in table), "no case takes the order by default (weights larger than the input)"


def test_plan_query_validates_like_the_launcher_and_follows_the_workspace(set_case_switches):
    from ctypes import byref
    L = importlib.import_module(R.PKG + "._lib")
    ops = importlib.import_module(R.PKG + ".ops")
    lib = L.load()
    p = L.GGPlan()
    assert lib.vg_gather_gemm_plan(byref(L.GGDesc()), G.BF16, byref(p)) == -1
    assert lib.vg_gather_gemm_plan(byref(L.GGDesc()), 7, byref(p)) == -3
    case = R.SPLITK[0]
    assert set_case_switches(case)["ksplit"] == 4
    g, _ = case.specs()
    unsplit = ops.gather_gemm_plan(g, case.dtype, bias=True, workspace=False)           # no workspace: the launcher does not split
    assert (unsplit["ksplit"], unsplit["reduce"], unsplit["stages_per_split"]) == (1, "none", 0) and unsplit["dma"]
    assert not ops.gather_gemm_plan(g, case.dtype, bias=True, zeros=False)["dma"]       # no zero page: register staging


# ---- the record against the side queries it replaced ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parent():
    """tools/gen_golden_gg_plan.py: the answers of the four side queries of vg_gather_gemm (slab count, tile rows, workspace
    bytes, timer family) and of the plan query, recorded at the last commit that had them."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gg_plan_parent.json")) as f:
        return json.load(f)


def _assert_reproduces(ops, rec, g, dtype, epi, where):
    plan = ops.gather_gemm_plan(g, dtype, **epi)
    got = (plan["nparts"], plan["bm"], plan["ws_bytes"], plan["timing_family"])
    assert got == (rec["nparts"], rec["tile_m"], rec["ws_bytes"], rec["family"]), (where, got, rec)
    old = dict(rec["plan"], detail=tuple(rec["plan"]["detail"]))
    assert {k: plan[k] for k in old} == old, (where, plan, old)
    # rows per statistics slab as engine.can_group asks for them (the old tile query on a statistics launch)
    assert ops.gather_gemm_plan(g, dtype, want_stats=True)["bm"] == rec["tile_m_stats"], where


@pytest.fixture
def default_switches(vg_switch, monkeypatch):
    for n in SWITCH_NAMES:
        monkeypatch.delenv(n, raising=False)
    ops = importlib.import_module(R.PKG + ".ops")
    ops.reload_switches()
    return ops


def test_plan_record_reproduces_the_side_queries_on_the_case_table(set_case_switches):
    ops = importlib.import_module(R.PKG + ".ops")
    recorded = _parent()["cases"]
    assert sorted(recorded) == sorted(R.ALL_IDS)
    for c in R.ALL_CASES:
        set_case_switches(c)
        _assert_reproduces(ops, recorded[c.id], c.specs()[0], c.dtype,
                           dict(bias=c.has("b"), want_stats=c.has("s"), act=c.act, mask=c.mask), c.id)
    assert sum(r["ws_bytes"] > 0 for r in recorded.values()) >= len(R.SPLITK)
    assert {r["family"] for r in recorded.values()} == {0, 2, 3}


@pytest.mark.parametrize("S,B,dtype", R.NETWORK_SHAPES, ids=[f"S{s}_B{b}_{d}" for s, b, d in R.NETWORK_SHAPES])
def test_plan_record_reproduces_the_side_queries_on_every_network_launch(S, B, dtype, default_switches):
    """Encoder, Generator and Discriminator (the latter also at 2B), forward and data gradient, the e4m3 operands where the
    engine takes them: what ops.gather_gemm now reads from ONE plan is what its four queries answered."""
    ops = default_switches
    recorded = _parent()["networks"][f"S{S}_B{B}_{dtype}"]
    launches = R.network_launches(S, B, dtype)
    assert sorted(recorded) == sorted(k for k, _, _, _ in launches)
    for key, g, kdt, epi in launches:
        _assert_reproduces(ops, recorded[key], g, kdt, epi, key)
    assert any(r["ws_bytes"] > 0 and r["plan"]["ksplit"] > 1 for r in recorded.values())
    assert (dtype == "fp8") == any(r["family"] == 3 for r in recorded.values())


@pytest.mark.parametrize("S,B,dtype", R.NETWORK_SHAPES, ids=[f"S{s}_B{b}_{d}" for s, b, d in R.NETWORK_SHAPES])
def test_can_group_answers_are_those_of_the_tile_query(S, B, dtype, default_switches):
    """The grouped Discriminator pass (groups = 2): tile rows per BatchNorm stage and the divisibility answer, re-derived
    from the plan, and what engine.StackEngine.can_group itself says -- host only, no tensor."""
    ops = default_switches
    rec = _parent()["can_group"][f"S{S}_B{B}_{dtype}"]
    stages = R.group_stages(S, B, dtype)
    assert [i for i, *_ in stages] == [s["stage"] for s in rec["stages"]]
    answer = True
    for (i, g, kdt, rows_per_group, plain), s in zip(stages, rec["stages"]):
        bm = ops.gather_gemm_plan(g, kdt, want_stats=True)["bm"]
        assert (bm, rows_per_group, plain) == (s["bm"], s["rows_per_group"], s["plain"]), (i, bm)
        answer = answer and plain and rows_per_group % bm == 0
    assert answer == rec["answer"]
    assert dict(R.build_networks(S, dtype))["D"]._engine.can_group(B, 2) == rec["answer"]


def test_plan_with_the_placeholder_workspace_is_the_plan_of_the_sized_launch(set_case_switches):
    """ops.gather_gemm asks once, before it has a workspace (non-NULL placeholder of 'enough' bytes), and then passes one of
    the plan's ws_bytes: both descriptors must give the same record, field for field; four bytes less and K is not split."""
    ops = importlib.import_module(R.PKG + ".ops")
    for c in R.SPLITK:
        asked = set_case_switches(c)
        epi = dict(bias=c.has("b"), want_stats=c.has("s"), act=c.act, mask=c.mask)
        g, _ = c.specs()
        assert asked["ksplit"] > 1 and asked["ws_bytes"] > 0 and asked["ws_bytes"] % 4 == 0, c.id
        assert ops.gather_gemm_plan(g, c.dtype, workspace=asked["ws_bytes"], **epi) == asked, c.id
        short = ops.gather_gemm_plan(g, c.dtype, workspace=asked["ws_bytes"] - 4, **epi)
        assert short["ksplit"] == 1 and short["reduce"] == "none" and short["ws_bytes"] == asked["ws_bytes"], c.id
        assert ops.gather_gemm_plan(g, c.dtype, workspace=False, **epi)["ws_bytes"] == asked["ws_bytes"], c.id
