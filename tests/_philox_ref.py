"""Host reference for the device generator: Philox4x32-10 from its published definition (Salmon, Moraes, Dror, Shaw:
"Parallel random numbers: as easy as 1, 2, 3", SC'11, section 3.3 and the Random123 constants), the project's packing of
(seed, step, draw, block) into counter and key as include/vaegan_hip.h states it ("In-kernel N(0,1) noise": word layout),
the 24-bit uniform, and Box-Muller in f64 on the f32-quantised inputs.  numpy only: no torch device, no project import.

One round of Philox-4x32 on counter (c0, c1, c2, c3) with round key (k0, k1):
    (hi0, lo0) = M0 * c0,  (hi1, lo1) = M1 * c2          (32 x 32 -> 64 bit products, split in halves)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
and between rounds the key is bumped by the Weyl constants (W0, W1).  Ten rounds."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # key increments: golden ratio, sqrt(3) - 1
ROUNDS = 10
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
N_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -33)))     # the largest |n| Box-Muller can give on u >= 2^-33
TWO_PI_F32 = np.float32(6.283185307179586)


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=ROUNDS):
    """-> (w0, w1, w2, w3) as uint32 arrays; every argument a 32-bit value (scalar or array, broadcast together)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) for v in (c0, c1, c2, c3, k0, k1)))
    for v in (c0, c1, c2, c3, k0, k1):
        assert not (v >> S32).any(), "counter and key words are 32-bit"
    m0, m1 = np.uint64(M0), np.uint64(M1)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
        p0, p1 = m0 * c0, m1 * c2                       # < 2^64: no wrap in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def counter(seed, step, draw, blk):
    """The project's packing -> (c0, c1, c2, c3, k0, k1).  Domain: draw in [0, 256), step < 2^56, seed and blk < 2^64."""
    seed, step, draw, blk = np.broadcast_arrays(*(_u64(v) for v in (seed, step, draw, blk)))
    assert (draw < np.uint64(256)).all() and not (step >> np.uint64(56)).any(), "draw in [0, 256), step < 2^56"
    c3 = (((step >> S32) << np.uint64(8)) | draw) & MASK
    return blk & MASK, blk >> S32, step & MASK, c3, seed & MASK, seed >> S32


def blocks(seed, step, draw, blk):
    """The four output words of block(s) blk, as a uint32 array [..., 4]."""
    return np.stack(philox4x32_10(*counter(seed, step, draw, blk)), axis=-1)


def words(seed, step, draw, n, start=0):
    """uint32 [n]: element i (i = start .. start + n - 1) is word i & 3 of block i >> 2."""
    i = np.arange(start, start + n, dtype=np.uint64)
    first, last = int(start) >> 2, (int(start) + n - 1) >> 2
    w = blocks(seed, step, draw, np.arange(first, last + 1, dtype=np.uint64)).reshape(-1)
    return w[(i - np.uint64(4 * first)).astype(np.int64)]


def u01(w):
    """(w >> 8) * 2^-24 in [0, 1): 24 significant bits, exact in float32."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def bm_inputs(wa, wb):
    """The f32 quantisation of one Box-Muller pair, every step one correctly rounded float32 operation:
    ua = max((f32(wa) + 0.5) * 2^-32, 1e-30) in (0, 1], t = f32(2 pi) * ((f32(wb) + 0.5) * 2^-32) in [0, f32(2 pi)]."""
    half, scale = np.float32(0.5), np.float32(2.0 ** -32)
    ua = (np.asarray(wa, dtype=np.uint32).astype(np.float32) + half) * scale
    ua = np.maximum(ua, np.float32(1e-30))
    ub = (np.asarray(wb, dtype=np.uint32).astype(np.float32) + half) * scale
    t = TWO_PI_F32 * ub
    assert ua.dtype == np.float32 and t.dtype == np.float32
    return ua, t


def randn_from_words(w):
    """w: whole blocks, uint32 [nb, 4] -> (normal, r, ua, t), each [nb, 4]; see randn_ref."""
    wa = np.stack([w[:, 0], w[:, 0], w[:, 2], w[:, 2]], axis=1)
    wb = np.stack([w[:, 1], w[:, 1], w[:, 3], w[:, 3]], axis=1)
    ua, t = bm_inputs(wa, wb)
    r = np.sqrt(-2.0 * np.log(ua.astype(np.float64))) + 0.0            # + 0.0: r = +0 at ua == 1, not -0
    t64 = t.astype(np.float64)
    trig = np.stack([np.cos(t64[:, 0]), np.sin(t64[:, 1]), np.cos(t64[:, 2]), np.sin(t64[:, 3])], axis=1)
    return r * trig, r, ua, t


def randn_ref(seed, step, draw, n):
    """-> (normal f64 [n], r f64 [n], ua f32 [n], t f32 [n]) of elements 0 .. n - 1: components 0, 1 of a block are
    r cos t, r sin t of the pair (w0, w1), components 2, 3 those of (w2, w3).  After the f32 quantisation of ua and t
    (bm_inputs) everything is f64."""
    nb = (n + 3) >> 2
    w = blocks(seed, step, draw, np.arange(nb, dtype=np.uint64))
    return tuple(a.reshape(-1)[:n] for a in randn_from_words(w))


def pair_words(seed, step, draw, idx):
    """(wa, wb) of the Box-Muller pair that element idx belongs to."""
    w = blocks(seed, step, draw, int(idx) >> 2)
    k = int(idx) & 2
    return int(w[k]), int(w[k + 1])


# ---- the cases the CPU and GPU tests share -------------------------------------------------------------------------------
KATS = (  # Random123 known-answer vectors for philox4x32-10 (kat_vectors): counter, key -> output
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

# One axis at a time around a default whose every word is non-zero, plus the all-zero key (the first KAT seen through >> 8).
D_SEED, D_STEP, D_DRAW, D_N = 0x0123456789ABCDEF, 0x00A5C3E19B7D2F01, 5, 4099
SIZES = (1, 3, 4, 5, 255, 256, 257, 4099, (1 << 20) + 5)        # the last one crosses the materialisers' 4096 x 256 stride
SEEDS = (0, 1, (1 << 32) - 1, 1 << 32, 0x0123456789ABCDEF, (1 << 63) - 1)
STEPS = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 56) - 1)
DRAWS = (0, 1, 2, 255)


def key_grid(extra_draws=()):
    """[(id, seed, step, draw, n)]: every value of each axis with the other axes at the default, and the all-zero case."""
    g = [("n=%d" % n, D_SEED, D_STEP, D_DRAW, n) for n in SIZES]
    g += [("seed=%#x" % s, s, D_STEP, D_DRAW, D_N) for s in SEEDS if s != D_SEED]
    g += [("step=%#x" % s, D_SEED, s, D_DRAW, D_N) for s in STEPS]
    g += [("draw=%d" % d, D_SEED, D_STEP, d, D_N) for d in tuple(DRAWS) + tuple(d for d in extra_draws if d not in DRAWS)]
    g.append(("zero", 0, 0, 0, 4))
    return g


# Box-Muller edge rows: (step, idx, class) at EDGE_SEED / EDGE_DRAW, idx < 4096 the cosine element of the pair.  Found by a
# search of steps 0 .. 65535 (2^26 blocks, 2^27 pairs) with this reference alone; every class was found as specified, none
# needed a lower bar.  Class (a) has probability 2^-25 per pair: the search met one such pair.
#   a   wa >= 2^32 - 128: f32(wa) = 2^32, ua = 1.0, r = 0, both normals are +-0
#   b   wa < 2^10: ua < 2^-22, r > 5.5 -- the far tail, near the 6.76 bound
#   c0 .. c4   |t - k pi / 2| < 2^-12 for k = 0 .. 4: the zero crossings of sine and cosine, both ends of the range
#              (row (4, 2280): wb >= 2^32 - 128, so t = f32(2 pi) itself)
#   d   wa in [2^23, 2^24): f32(wa) + 0.5 is rounded, not exact
EDGE_SEED, EDGE_DRAW, EDGE_N = 20240607, 5, 4096
EDGE_ROWS = (
    (5271, 3036, "a"),
    (3019, 122, "b"), (3106, 2792, "b"), (5545, 2530, "b"), (5673, 3884, "b"),
    (1, 1532, "c0"), (23, 1256, "c0"), (3, 2858, "c1"), (5, 410, "c1"), (4, 694, "c2"), (6, 1948, "c2"),
    (5, 3108, "c3"), (6, 4056, "c3"), (4, 2280, "c4"), (47, 3936, "c4"),
    (0, 974, "d"), (0, 2658, "d"),
)
EDGE_CLASSES = ("a", "b", "c0", "c1", "c2", "c3", "c4", "d")


def edge_class_holds(cls, wa, wb):
    if cls == "a":
        return wa >= 2 ** 32 - 128
    if cls == "b":
        return wa < 2 ** 10
    if cls == "d":
        return 2 ** 23 <= wa < 2 ** 24
    _, t = bm_inputs(np.uint32(wa), np.uint32(wb))
    return abs(float(t) - int(cls[1]) * np.pi / 2) < 2.0 ** -12


def header_draw_ids(header_text):
    """{name: id} of every `#define VG_DRAW_*` in include/vaegan_hip.h."""
    import re
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(VG_DRAW_\w+)\s+(\d+)\s*$", header_text, re.M)}
