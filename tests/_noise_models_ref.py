"""Host restatement of the noise models of the degraded pairs (include/vaegan_hip.h "Degraded pairs", noise models) and of the
median baseline ("Median baseline").  numpy only, f32 throughout, ONE rounding per operation: every intermediate below is a
float32 array, so numpy rounds each product, sum, quotient and root on its own, as the contract demands.  The draws come in
as arrays (materialised by the device or made on the host from tests/_philox_ref.py); nothing here imports the project."""
import numpy as np

import _philox_ref as P

GAUSSIAN, SPECKLE, SHOT = 0, 1, 2
KINDS = {"gaussian": GAUSSIAN, "speckle": SPECKLE, "shot": SHOT}
DRAW_NORMAL, DRAW_FILL, DRAW_PARAMS, DRAW_IMPULSE, DRAW_SALT = 16, 17, 18, 19, 20
F = np.float32


def degrade_ref(clean, n, s, noise_max_std, kind, normalize, fill=None, rect=None, impulse_u=None, salt_u=None,
                impulse_max_p=0.0, salt_ratio=0.5):
    """One image.  clean, n (and fill, impulse_u, salt_u where used): f32 [C,H,W]; s: the image's severity; rect: None or
    (rect_h, rect_w, x, y); kind: 0 / 1 / 2.  -> f32 [C,H,W]."""
    clean, n = np.asarray(clean, F), np.asarray(n, F)
    assert clean.dtype == F and n.dtype == F
    s, nms = F(s), F(noise_max_std)
    base = clean.copy()
    if rect is not None:
        rh, rw, x, y = rect
        f = np.asarray(fill, F)[:, y:y + rh, x:x + rw]
        base[:, y:y + rh, x:x + rw] = f * F(2.0) - F(1.0)
    lo, span = (F(-1.0), F(2.0)) if normalize else (F(0.0), F(1.0))
    level = (n * s) * nms
    if kind == GAUSSIAN:
        t = base + level
    else:
        g = np.maximum((base - lo) / span, F(0.0))
        f = g if kind == SPECKLE else np.sqrt(g)
        assert f.dtype == F
        t = base + level * f
    t = np.minimum(np.maximum(t, F(-1.0)), F(1.0))
    assert t.dtype == F
    if impulse_max_p > 0:
        p_b = s * F(impulse_max_p)
        hit = np.asarray(impulse_u, F) < p_b
        salt = np.asarray(salt_u, F) < F(salt_ratio)
        t = np.where(hit, np.where(salt, F(1.0), lo), t).astype(F)
    return t


def severity(seed, pos):
    """s of the image at epoch position pos: u01 of word 0 of draw VG_DRAW_DEGRADE_PARAMS."""
    return P.u01(P.words(seed, pos, DRAW_PARAMS, 1))[0]


def impulse_masks(seed, pos, n_elements, impulse_max_p, salt_ratio):
    """(hit, salt) bool [n_elements] of the image at (seed, pos) from host Philox words alone: hit where the impulse uniform is
    below p_b = s * impulse_max_p, salt where a HIT element's salt uniform is below salt_ratio (else pepper).  -> also p_b."""
    p_b = severity(seed, pos) * F(impulse_max_p)
    hit = P.u01(P.words(seed, pos, DRAW_IMPULSE, n_elements)) < p_b
    salt = hit & (P.u01(P.words(seed, pos, DRAW_SALT, n_elements)) < F(salt_ratio))
    return hit, salt, p_b


def median_ref(x, r):
    """x: [..., H, W]; the (2r+1)^2 median of the last two axes, np.pad(mode="reflect") at the border, by sorting."""
    x = np.asarray(x)
    H, W = x.shape[-2:]
    pad = [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)]
    xp = np.pad(x, pad, mode="reflect")
    k = 2 * r + 1
    wins = np.stack([xp[..., i:i + H, j:j + W] for i in range(k) for j in range(k)], axis=-1)
    return np.sort(wins, axis=-1)[..., (k * k) // 2]
