"""A float64 restatement of the atlas modes of the reference's fragment shader (atlas.frag: mode 0, the image, and modes 13 - 16, the
multi-channel distance fields) for ONE upright quad over a clear colour -- the second witness of the frames that have no golden
(tests/hostile_atlas_cases.ORACLE_ONLY).  Plain numpy; it shares no code with oracle/figdraw_oracle.c or oracle/ref_swiftshader.py.

What it states, from the shader and the GL pipeline around it:
  * the atlas: every image at its rectangle on level 0, its chain of 2 x 2 box means (sum div 4; an odd extent keeps a half-covered
    last column / row) at (x >> l, y >> l) while both extents exceed 1; a chain given level by level goes in as it is
  * the quad: corners transformed in float32 and snapped up to whole pixels, uv linear between them, a fragment per pixel centre inside
  * texture(): level of detail log2(rho), rho the larger axis' texels per pixel, clamped to the chain; LINEAR within a level, REPEAT at
    its border, LINEAR between two levels; magnified: level 0.  textureLod(.., 0) for the distance fields
  * median of three, screenPxRange = max(0.5 (unit / fwidth(u) + unit / fwidth(v)), 1), the fill alpha clamp(spr (sd - threshold) + 0.5)
    and the stroke alpha clamp(w / 2 - |spr (sd - threshold)| + 0.5)
  * vertex colours interpolated over the triangles (TL, BL, BR) and (TR, TL, BR)
  * the blend SRC_ALPHA, ONE_MINUS_SRC_ALPHA (alpha: ONE, ONE_MINUS_SRC_ALPHA) onto the clear colour as the 8-bit surface holds it, and
    rounding to RGBA8"""
import numpy as np

f32 = np.float32


def minify(img):
    """the next level of an RGBA8 image: 2 x 2 sums div 4; an odd extent rounds the size up and the extra column / row is the mean of the
    last one's pairs at half coverage ((127 a + 128 b) div 255, then (128 v) div 255), the extra corner a quarter ((64 v) div 255)"""
    a = img.astype(np.int64)
    h, w = a.shape[:2]
    eh, ew = h // 2, w // 2
    out = np.zeros(((h + 1) // 2, (w + 1) // 2, 4), np.int64)
    out[:eh, :ew] = (a[0:2 * eh:2, 0:2 * ew:2] + a[0:2 * eh:2, 1:2 * ew:2] + a[1:2 * eh:2, 0:2 * ew:2] + a[1:2 * eh:2, 1:2 * ew:2]) // 4
    if w % 2:
        out[:eh, ew] = ((a[0:2 * eh:2, w - 1] * 127 + a[1:2 * eh:2, w - 1] * 128) // 255) * 128 // 255
    if h % 2:
        out[eh, :ew] = ((a[h - 1, 0:2 * ew:2] * 127 + a[h - 1, 1:2 * ew:2] * 128) // 255) * 128 // 255
        if w % 2:
            out[eh, ew] = a[h - 1, w - 1] * 64 // 255
    return out.astype(np.uint8)


def build_atlas(images, rects, size):
    """the levels of an atlas of `size` that holds `images` (key -> array, or a list of arrays: its levels) at `rects` (key -> x, y, w, h)"""
    n = int(np.log2(size)) + 1
    levels = [np.zeros((size >> l, size >> l, 4), np.uint8) for l in range(n)]

    def store(l, x, y, img):
        ls = size >> l
        hh, ww = min(img.shape[0], ls - y), min(img.shape[1], ls - x)
        if hh > 0 and ww > 0:
            levels[l][y:y + hh, x:x + ww] = img[:hh, :ww]

    for k in sorted(images):
        x, y = rects[k][:2]
        if isinstance(images[k], (list, tuple)):
            for l, img in enumerate(images[k][:n]):
                store(l, x >> l, y >> l, np.asarray(img))
            continue
        img, l = np.asarray(images[k]), 0
        while img.shape[0] > 1 and img.shape[1] > 1 and l < n:
            store(l, x, y, img)
            img, x, y, l = minify(img), x // 2, y // 2, l + 1
    return levels


def _bilinear(level, u, v):
    """LINEAR, REPEAT: u, v normalised float64 arrays -> (.., 4) float64 in 0 .. 1"""
    s = level.shape[0]
    x, y = u * s - 0.5, v * s - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    x0, y0 = x0.astype(np.int64) % s, y0.astype(np.int64) % s
    x1, y1 = (x0 + 1) % s, (y0 + 1) % s
    t = level.astype(np.float64) / 255.0
    top = t[y0, x0] * (1.0 - ax) + t[y0, x1] * ax
    bot = t[y1, x0] * (1.0 - ax) + t[y1, x1] * ax
    return top * (1.0 - ay) + bot * ay


def render_quad(call, levels, rects, w, h, clear, xf=None, subpixel=None):
    """the frame (h x w x 4 uint8) of one draw_image / draw_image_adj / draw_msdf call (the call-stream form) over `clear`, drawn under the
    transform xf = (sx, sy, tx, ty); subpixel: the sub-pixel shift if the context's switch is on"""
    size = levels[0].shape[0]
    name, key, pos = call[0], call[1], call[2]
    ex, ey, ew, eh = rects[key]
    u_at, v_at, u_to, v_to = ex / size, ey / size, (ex + ew) / size, (ey + eh) / size
    if name == "draw_image":
        cols, dim, flip = call[3], call[4], call[5]
        if not (dim[0] > 0 and dim[1] > 0):
            dim = [float(ew), float(eh)]
        mode = 0
    elif name == "draw_image_adj":
        cols, dim, flip, mode = [call[3]] * 4, call[4], 0, 0
        u_at, v_at, u_to, v_to = u_at + 2.0 / size, v_at + 2.0 / size, u_to - 2.0 / size, v_to - 2.0 / size
    else:
        assert name == "draw_msdf"
        cols, dim, px_range, thr, sw, mtsdf, flip = [call[3]] * 4, call[4], call[5], call[6], max(call[7], 0.0), call[8], call[9]
        px_range, thr, sw = float(f32(px_range)), float(f32(thr)), float(f32(sw))
        mode = (16 if sw > 0 else 14) if mtsdf else (15 if sw > 0 else 13)
    if flip:
        v_at, v_to = v_to, v_at
    sx, sy, tx, ty = (f32(v) for v in (xf or (1.0, 1.0, 0.0, 0.0)))
    x_at, y_at = f32(pos[0]), f32(pos[1])
    x_to, y_to = f32(x_at + f32(dim[0])), f32(y_at + f32(dim[1]))
    X_at, X_to = float(np.ceil(f32(sx * x_at) + tx)), float(np.ceil(f32(sx * x_to) + tx))  # (an upright transform: one product, one sum)
    Y_at, Y_to = float(np.ceil(f32(sy * y_at) + ty)), float(np.ceil(f32(sy * y_to) + ty))
    out = np.empty((h, w, 4), np.float64)
    out[:] = np.floor(np.asarray(clear, np.float64) * 255.0 + 0.5) / 255.0
    i0, i1 = int(max(min(X_at, X_to), 0)), int(min(max(X_at, X_to), w))
    j0, j1 = int(max(min(Y_at, Y_to), 0)), int(min(max(Y_at, Y_to), h))
    if i1 > i0 and j1 > j0 and X_at != X_to and Y_at != Y_to:
        s = ((np.arange(i0, i1) + 0.5 - X_at) / (X_to - X_at))[None, :] * np.ones((j1 - j0, 1))
        t = ((np.arange(j0, j1) + 0.5 - Y_at) / (Y_to - Y_at))[:, None] * np.ones((1, i1 - i0))
        u, v = u_at + (u_to - u_at) * s, v_at + (v_to - v_at) * t
        dudx, dvdy = abs((u_to - u_at) / (X_to - X_at)), abs((v_to - v_at) / (Y_to - Y_at))
        c = np.asarray(cols, np.float64) / 255.0  # BL, BR, TR, TL
        bl, br, tr, tl = c[0], c[1], c[2], c[3]
        s3, t3 = s[..., None], t[..., None]
        col = np.where(t3 >= s3, tl * (1.0 - t3) + bl * (t3 - s3) + br * s3, tl * (1.0 - s3) + tr * (s3 - t3) + br * t3)
        if mode == 0:
            if subpixel is not None:
                u = u - min(max(float(f32(subpixel)), 0.0), float(f32(0.999))) / size
            rho = max(dudx, dvdy) * size
            lam = np.log2(rho) if rho > 0 else 0.0
            if lam <= 0.0:
                tex = _bilinear(levels[0], u, v)
            else:
                lam = min(lam, float(len(levels) - 1))
                l0 = int(np.floor(lam))
                l1 = min(l0 + 1, len(levels) - 1)
                f = lam - l0
                tex = _bilinear(levels[l0], u, v) * (1.0 - f) + _bilinear(levels[l1], u, v) * f
            src = tex * col
        else:
            tex = _bilinear(levels[0], u, v)
            sd = tex[..., 3] if mode in (14, 16) else np.maximum(np.minimum(tex[..., 0], tex[..., 1]), np.minimum(np.maximum(tex[..., 0], tex[..., 1]), tex[..., 2]))
            unit = px_range / size
            spr = max(0.5 * (unit / dudx + unit / dvdy), 1.0) if dudx > 0 and dvdy > 0 else 1.0
            spd = spr * (sd - thr)
            alpha = np.clip(0.5 * sw - np.abs(spd) + 0.5, 0.0, 1.0) if mode in (15, 16) else np.clip(spd + 0.5, 0.0, 1.0)
            src = col.copy()
            src[..., 3] = col[..., 3] * alpha
        dst = out[j0:j1, i0:i1]
        sa = src[..., 3:4]
        dst[..., :3] = src[..., :3] * sa + dst[..., :3] * (1.0 - sa)
        dst[..., 3:4] = sa + dst[..., 3:4] * (1.0 - sa)
    return np.floor(np.clip(out, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
