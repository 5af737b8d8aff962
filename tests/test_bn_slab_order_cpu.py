"""CPU: the inputs of tests/test_gpu_bn_slab_order.py can tell summation orders apart, and tests/_bn_slab_ref.py's vectorised
orders are the scalar loops they claim to be."""
import numpy as np
import pytest

import _bn_slab_ref as S

f32, f64 = np.float32, np.float64


def _cases():
    return [("ff",) + c for c in S.FUSED_CASES] + [("fin",) + c for c in S.FIN_CASES]


def _both(kind, C, groups, nparts):
    seed = S.seed_of(kind, C, groups, nparts)
    return S.fwd_case(seed, groups, nparts, C), S.bwd_case(seed, groups, nparts, C)


@pytest.mark.parametrize("kind,C,groups,nparts", _cases(), ids=lambda v: str(v))
def test_row_order_gives_other_bits(kind, C, groups, nparts):
    """Every case, forward and backward slabs, every group: the f32 casts of the sums in plain row order differ from the
    kernel's order in at least one channel -- wherever the two orders are different additions at all (more than 16 rows for
    the one-launch forms, more than 3 for the finalize kernels; up to there they are the same adds and must give the same
    bits).  Also: more than 40 binades between the smallest and the largest slab value, and a positive variance everywhere."""
    fw, bw = _both(kind, C, groups, nparts)
    for d in (fw, bw):
        ordered, plain = S.ORDER[kind](d["slabs"]), S.row_sums(d["slabs"])
        if nparts > S.SAME_AS_ROW_UP_TO[kind]:
            assert S.differs(ordered, plain).all(), "row order gives the kernel's bits: the case proves nothing"
        else:
            assert all((u.view(np.uint64) == v.view(np.uint64)).all() for u, v in zip(ordered, plain))
        if nparts >= 3:
            a = np.abs(d["slabs"].astype(f64))
            assert np.log2(a.max() / a.min()) > 40
    count = S.FIN_COUNT if kind == "fin" else S.FUSED_RPG[0]
    s1, s2 = S.ORDER[kind](fw["slabs"])
    assert (s2 / count - (s1 / count) ** 2 > 0).all()


def _scalar_ff(col):
    lanes = [0.0] * 16
    for pl in range(16):
        for p in range(pl, len(col), 16):
            lanes[pl] += float(col[p])
    s = 0.0
    for v in lanes:
        s += v
    return s


def _scalar_fin(col):
    planes = [0.0] * 128
    for pl in range(128):
        for p in range(pl, len(col), 128):
            planes[pl] += float(col[p])
    waves = []
    for w in range(16):
        a = planes[8 * w:8 * w + 8]
        waves.append(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])))
    s = waves[0]
    for v in waves[1:]:
        s += v
    return s


@pytest.mark.parametrize("kind,nparts", [("ff", 17), ("ff", 200), ("fin", 129), ("fin", 1300)])
def test_vectorised_orders_are_the_scalar_loops(kind, nparts):
    slabs = S.bwd_case(5, 2, nparts, 8)["slabs"]
    got = S.ORDER[kind](slabs)
    one = _scalar_ff if kind == "ff" else _scalar_fin
    for g in range(2):
        for k in range(2):
            for c in range(8):
                assert got[k][g, c] == one(slabs[g, :, k, c])


def test_single_rounding_helper():
    a, b, c = f32(1 + 2.0 ** -23), f32(1 + 2.0 ** -23), f32(2.0 ** -30)
    # a * b = 1 + 2^-22 + 2^-46: c - a*b in one rounding is -(1 + 2^-22); product rounded first gives the same here, so use a tie
    assert S.fma_neg(np.array([a]), np.array([b]), np.array([c]))[0] == f32(-(1 + 2.0 ** -22))
    # tie broken by the sticky bits only an exact product keeps: 3 * (1 + 2^-23) = 3 + 3 * 2^-23, halfway is 3 + 2^-22 + 2^-23
    x, y = f32(3.0), f32(1 + 2.0 ** -23)
    assert S.fma_neg(np.array([x]), np.array([y]), np.array([f32(0)]))[0] == f32(-(3 + 2.0 ** -21))
