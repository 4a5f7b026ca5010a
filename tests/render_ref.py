"""numpy restatement of skp_map_range / skp_render_sheet (include/skp.h, A17) and the shared
cases and comparison rule of tests/test_render_cpu.py and tests/test_gpu_render.py.

The restatement runs in any float type: float64 is the reference of the GPU test, float32
against float64 shows without a GPU that the test inputs satisfy the rule's conditions.
"""
import numpy as np

TAU = 0.01          # counts: a byte may differ by one where the pre-rounding value is this close to k + 0.5
MIN_RANGE = 1e-3    # every non-constant test map spans at least this
MIN_MARGIN = 1e-3   # pixels: no pixel centre is closer than this to a marker circle
MAX_BAND = 0.05     # share of bytes inside the ±TAU band (a uniform fractional part gives 2·TAU)

PAD, EMPTY, DISC, OUTLINE, PLAIN, HEAT = range(6)


def map_range_ref(maps):
    """(n, h, w) float32 -> (n, 2) float32: (min, max), or NaN for a non-finite or constant map."""
    out = np.full((maps.shape[0], 2), np.nan, np.float32)
    for i, m in enumerate(maps):
        if np.isfinite(m).all() and m.max() != m.min():
            out[i] = m.min(), m.max()
    return out


def _taps(n_out, n_in, dt):
    src = np.maximum(dt(n_in) / dt(n_out) * (np.arange(n_out, dtype=dt) + dt(0.5)) - dt(0.5), dt(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (src - i0.astype(dt)).astype(dt)
    return i0, i1, dt(1) - w1, w1


def render_ref(images, maps, rng, lut, alpha, points, radius, colors, rows, cols, f, pad, dtype=np.float64):
    """Returns (bytes (Hs, Ws, 3) uint8, pre (Hs, Ws, 3) pre-rounding counts (NaN where the byte is
    fixed), kind (Hs, Ws) of PAD … HEAT, margin = least distance of a pixel centre to a marker circle)."""
    dt = dtype
    n, _, H, W = images.shape
    th, tw = H // f, W // f
    Hs, Ws = rows * (th + pad) + pad, cols * (tw + pad) + pad
    out = np.full((Hs, Ws, 3), 255, np.uint8)
    pre = np.full((Hs, Ws, 3), np.nan, dt)
    kind = np.full((Hs, Ws), PAD, np.int64)
    margin = np.inf
    a = dt(np.float32(alpha))
    r = dt(np.float32(radius)) if radius is not None else dt(0)
    for t in range(rows * cols):
        y0, x0 = pad + (t // cols) * (th + pad), pad + (t % cols) * (tw + pad)
        if t >= n:
            kind[y0:y0 + th, x0:x0 + tw] = EMPTY
            continue
        comp = images[t].astype(dt)
        heat = maps is not None and not np.isnan(rng[t]).any()
        if heat:
            M = maps[t].astype(dt)
            mn, mx = dt(rng[t, 0]), dt(rng[t, 1])
            yi0, yi1, yw0, yw1 = _taps(H, M.shape[0], dt)
            xi0, xi1, xw0, xw1 = _taps(W, M.shape[1], dt)
            m = (yw0[:, None] * (xw0 * M[yi0][:, xi0] + xw1 * M[yi0][:, xi1]) +
                 yw1[:, None] * (xw0 * M[yi1][:, xi0] + xw1 * M[yi1][:, xi1]))
            v = np.clip((m - mn) / (mx - mn), dt(0), dt(1))
            x = dt(255) * v
            i0 = np.clip(np.floor(x).astype(np.int64), 0, 255)
            i1 = np.minimum(i0 + 1, 255)
            fr = (x - i0.astype(dt))[None]
            L = lut.astype(dt)
            l0, l1 = L[i0].transpose(2, 0, 1), L[i1].transpose(2, 0, 1)
            comp = (dt(1) - a) * comp + a * (l0 + fr * (l1 - l0))
        c = comp.reshape(3, th, f, tw, f).sum(axis=(2, 4), dtype=dt) / dt(f * f)
        p = (np.clip(c, dt(0), dt(1)) * dt(255)).transpose(1, 2, 0)
        tile = np.floor(p + dt(0.5)).astype(np.uint8)
        k = np.full((th, tw), HEAT if heat else PLAIN, np.int64)
        if points is not None and points.shape[1] > 0:
            yy = (np.arange(th, dtype=dt) + dt(0.5))[:, None]
            xx = (np.arange(tw, dtype=dt) + dt(0.5))[None, :]
            for j in range(points.shape[1]):
                py, px = dt(points[t, j, 0]) * dt(th), dt(points[t, j, 1]) * dt(tw)
                with np.errstate(invalid="ignore"):
                    d2 = (yy - py) ** 2 + (xx - px) ** 2
                    disc = d2 <= r * r
                    ring = ~disc & (d2 <= (r + dt(1)) * (r + dt(1)))
                    if np.isfinite(d2).all():
                        d = np.sqrt(d2.astype(np.float64))
                        margin = min(margin, np.abs(d - float(r)).min(), np.abs(d - float(r) - 1.0).min())
                tile[disc] = colors[j]
                tile[ring] = 255
                k[disc], k[ring] = DISC, OUTLINE
                p = np.where((disc | ring)[..., None], np.nan, p)
        out[y0:y0 + th, x0:x0 + tw] = tile
        pre[y0:y0 + th, x0:x0 + tw] = p
        kind[y0:y0 + th, x0:x0 + tw] = k
    return out, pre, kind, margin


def in_band(pre):
    """Bytes whose pre-rounding value lies within TAU of a half-integer."""
    with np.errstate(invalid="ignore"):
        return np.abs(pre - np.floor(pre) - 0.5) <= TAU


def check(got, ref, f):
    """The rule: ``got`` equals the reference bytes everywhere, except that inside the ±TAU band a
    difference of one count is allowed; padding, the empty tile, disc and outline pixels, and
    no-overlay pixels at f = 1 are exact with no exemption."""
    rb, pre, kind, _ = ref
    diff = np.abs(got.astype(np.int64) - rb.astype(np.int64))
    exact = np.isin(kind, (PAD, EMPTY, DISC, OUTLINE)) | ((kind == PLAIN) & (f == 1))
    assert got.shape == rb.shape
    assert (diff[exact] == 0).all(), f"{int((diff[exact] != 0).sum())} bytes differ where none may"
    band = in_band(pre) & ~exact[..., None]
    assert (diff[~band] == 0).all(), f"{int((diff[~band] != 0).sum())} bytes differ outside the band"
    assert diff.max() <= 1


def check_conditions(case, ref):
    """What keeps the rule honest, asserted on the restatement alone."""
    _, pre, _, margin = ref
    if case["maps"] is not None:
        for m in case["maps"]:
            if np.isfinite(m).all() and m.max() != m.min():
                assert m.max() - m.min() >= MIN_RANGE
    assert margin >= MIN_MARGIN, margin
    assert in_band(pre).mean() < MAX_BAND, in_band(pre).mean()


# ------------------------------------------------------------------------------------------ cases
# all: n = 5 images on 2 × 3 tiles (one empty tile), K = 5 markers of radius 2
CASES = {
    "a_f1_maps16": dict(H=16, f=1, pad=1, hw=(16, 16), heat=True, pts=True),
    "b_f2_maps8_upsampled": dict(H=16, f=2, pad=2, hw=(8, 8), heat=True, pts=True),
    "c_h12_maps5x7_odd_width": dict(H=12, f=1, pad=1, hw=(5, 7), heat=True, pts=True),
    "d_points_only": dict(H=16, f=1, pad=1, hw=None, heat=False, pts=True),
    "e_heat_only": dict(H=16, f=1, pad=1, hw=(16, 16), heat=True, pts=False),
    "f_overlay_mask_const_nan": dict(H=16, f=2, pad=1, hw=(16, 16), heat=True, pts=True, special=True),
    # a 23 × 34 sheet: four-pixel groups cross row ends and two pixels are left for the scalar tail
    "g_h10_width34_scalar_tail": dict(H=10, f=1, pad=1, hw=(5, 7), heat=True, pts=True),
}
N, ROWS, COLS, K, RADIUS, ALPHA = 5, 2, 3, 5, 2.0, 0.7
COLORS = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189)], np.uint8)


def _circle_margin(p, th):
    c = np.arange(th) + 0.5
    d = np.sqrt((c[:, None] - float(p[0]) * th) ** 2 + (c[None, :] - float(p[1]) * th) ** 2)
    return min(np.abs(d - RADIUS).min(), np.abs(d - RADIUS - 1.0).min())


def make_case(name, lut, seed=0):
    """Seeded inputs of one case.  Images are multiples of 1/4096, so image·255 + 0.5 (and the
    mean of 2×2 of them) is exact in float32 and the no-overlay bytes cannot depend on rounding."""
    spec = CASES[name]
    g = np.random.default_rng([seed, sorted(CASES).index(name)])
    H = spec["H"]
    images = (g.integers(0, 4097, (N, 3, H, H)) / 4096.0).astype(np.float32)
    maps = overlay = points = None
    if spec["heat"]:
        maps = g.random((N,) + spec["hw"]).astype(np.float32)
        if spec.get("special"):
            maps[1] = 0.25                      # constant: no overlay
            maps[3, 2, 3] = np.nan              # NaN: no overlay
            overlay = np.array([True, True, False, True, True])
    if spec["pts"]:
        base = np.array([(0.05, 0.07),          # within `radius` of the tile corner: clipped
                         (np.nan, 0.5),         # paints nothing
                         (0.53, 0.47), (0.60, 0.55),   # overlap: the later wins
                         (0.30, 0.80)], np.float32)
        th = H // spec["f"]
        points = np.empty((N, K, 2), np.float32)
        for t in range(N):
            for j in range(K):   # jitter redrawn until no pixel centre is near the two circles
                while True:
                    points[t, j] = base[j] + g.uniform(-0.02, 0.02, 2).astype(np.float32)
                    if np.isnan(points[t, j]).any() or _circle_margin(points[t, j], th) >= 10 * MIN_MARGIN:
                        break
    rng = None
    if maps is not None:
        rng = map_range_ref(maps)
        if overlay is not None:
            rng[~overlay] = np.nan
    return dict(name=name, images=images, maps=maps, overlay=overlay, points=points, rng=rng, lut=lut, f=spec["f"],
                pad=spec["pad"])


def reference(case, dtype=np.float64):
    return render_ref(case["images"], case["maps"], case["rng"], case["lut"], ALPHA, case["points"],
                      RADIUS if case["points"] is not None else None, COLORS, ROWS, COLS, case["f"], case["pad"],
                      dtype=dtype)
