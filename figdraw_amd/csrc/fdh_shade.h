// fdh_shade.h -- the compositor's generic per-pixel shading of one draw (shade_one) and the fill evaluation it uses, shared by the
// compositor (k_composite.hip: the one-pixel-slot path and the edge paths' gradients) and the hit-testing kernels (k_pick.hip), so that a
// pick sees exactly the source alpha the compositor blends with.
#pragma once
#include "fdh_device.h"

namespace fdh {

// evalFillColor atlas.frag:233-250, select-based.  Everything is passed BY VALUE: `c ? a.x : b.x` on lvalues is an
// lvalue conditional (pointer select, then a load), which pins arrays of F4 in scratch.
__device__ __forceinline__ float selectf(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ float fill_t(uint32_t fill_mode, float u, float v) {  // the gradient parameter, clamped (atlas.frag:236-243)
  float t;
  switch (fill_mode) {  // wave-uniform
    case 1u: t = u; break;
    case 2u: t = v; break;
    case 3u: t = 0.5f * (u + v); break;
    default: t = 0.5f * (u + (1.0f - v)); break;
  }
  return clamp01(t);
}
__device__ __forceinline__ F4 eval_fill_nb(F4 col, F4 m, F4 s, uint32_t fill_mode, float mid, float u, float v) {
  const float t = fill_t(fill_mode, u, v);
  const bool lo = t <= mid;
  const float w = selectf(lo, t * frcp(mid), (t - mid) * frcp(1.0f - mid));
  F4 o;
  o.x = mixf(selectf(lo, col.x, m.x), selectf(lo, m.x, s.x), w);
  o.y = mixf(selectf(lo, col.y, m.y), selectf(lo, m.y, s.y), w);
  o.z = mixf(selectf(lo, col.z, m.z), selectf(lo, m.z, s.z), w);
  o.w = mixf(selectf(lo, col.w, m.w), selectf(lo, m.w, s.w), w);
  return o;
}

__device__ __forceinline__ F4 eval_fill_rec(const DrawRec& r, F4 col, uint32_t fill_mode, float u, float v) {
  if (fill_mode == 0u) return col;
  const float k = 1.0f / 255.0f;
  const F4 mc = unpack255(r.mid), sc = unpack255(r.stop);
  const F4 m01 = {mc.x * k, mc.y * k, mc.z * k, mc.w * k}, s01 = {sc.x * k, sc.y * k, sc.z * k, sc.w * k};
  return eval_fill_nb(col, m01, s01, fill_mode, __builtin_fminf(__builtin_fmaxf(r.f1, 0.01f), 0.99f), u, v);
}

// The fragment of a rotated / skewed quad whose edge functions fit 32 bits (F_EDGE32) as the compositor's 4-wide paths form it, for the
// hit-testing kernels (k_pick.hip), which shade every draw through shade_one: those paths take a one-colour quad's colour from its
// first vertex (the device form of such a record holds floats in the other three, Recorder::commit_bins), and a bezier stroke's uv
// from barycentrics divided in double precision (tri_bary(exact) in k_composite_strip.inc: the closed-form cubic turns a last-bit
// difference of its input into pixels).  Every other record: make_frag.
__device__ __forceinline__ Frag make_frag_edge32(const DrawRec& r, const QuadExt* __restrict__ exts, int px, int py) {
  Frag f = make_frag(r, exts, px, py);
  const uint32_t om = r.op_mode, mode = om & 255u;
  if (!(om & F_GENERAL) || !(om & F_EDGE32)) return f;
  if (om & F_SOLID) {
    const F4 c = unpack255(r.col[0]);
    const float k = 1.0f / 255.0f;
    f.col = {c.x * k, c.y * k, c.z * k, c.w * k};
  }
  if (mode >= 18u && mode <= 20u) {
    const QuadExt& q = exts[r.ext];
    const long long X = 2 * px + 1, Y = 2 * py + 1;
    int hit = -1;
    long long e[3] = {0, 0, 0};
    for (int t = 0; t < 2; t++) {
      if (hit >= 0 || q.inv_sum[t] == 0.0f) continue;
      long long a[3];
      bool in = true;
      for (int k = 0; k < 3; k++) {
        a[k] = (long long)q.e[t][k].a * X + (long long)q.e[t][k].b * Y + q.e[t][k].c;
        in = in && (a[k] > 0 || (a[k] == 0 && ((q.own >> (t * 3 + k)) & 1u)));
      }
      if (in) { hit = t; e[0] = a[0]; e[1] = a[1]; e[2] = a[2]; }
    }
    if (hit >= 0) {
      const double inv = 1.0 / (double)(e[0] + e[1] + e[2]);
      const float l0 = (float)((double)e[0] * inv), l1 = (float)((double)e[1] * inv), l2 = (float)((double)e[2] * inv);
      const float sum = (hit == 1 ? l0 : l1) + l2;  // tri 0 = (TL, BL, BR): u = l2, v = l1 + l2;  tri 1 = (TR, TL, BR): u = l0 + l2, v = l2
      f.u = hit == 1 ? sum : l2;
      f.v = hit == 1 ? l2 : sum;
    }
  }
  return f;
}

// ---- generic one-pixel shading (atlas / MSDF sampling, rotated or skewed quads, rect-mask setup): the rare draws.
// Reads the record through the global pointer (dynamic field selection must not force a local copy into scratch).
// kPick: the hit-testing kernels' form -- the fragment as the compositor's 4-wide paths form it (make_frag_edge32).
struct Src { float r, g, b, a; bool covered; };
template <bool kPick = false>
__device__ __forceinline__ Src shade_one(const DrawRec* __restrict__ rp, const QuadExt* __restrict__ exts, const AtlasView* __restrict__ atlas,
                                      const uint32_t* __restrict__ backdrop, size_t pix, bool in_frame, int px, int py, F4 F) {
  const DrawRec& r = *rp;
  const uint32_t om = r.op_mode;
  const uint32_t mode = om & 255u;
  const bool ellip = (om & F_ELLIP) != 0u;
  const uint32_t fill_mode = (om >> 9) & 7u;
  const Frag f = kPick ? make_frag_edge32(r, exts, px, py) : make_frag(r, exts, px, py);
  Src s;
  s.covered = f.covered;
  if (((om >> 12) & 15u) == OP_MASK_PUSH) {  // mask.frag:186-234: returns the shape alpha (x colour alpha) in .a
    const float lx = (f.u - 0.5f) * 2.0f * r.p0, ly = (f.v - 0.5f) * 2.0f * r.p1;
    const float dist = shape_dist(ellip, lx, -ly, r.p2, r.p3, r.r[0], r.r[1], r.r[2], r.r[3]);
    s.r = s.g = s.b = 0.0f;
    s.a = (1.0f - clamp01(r.aa * dist + 0.5f)) * f.col.w;
    return s;
  }
  if (mode == 0u) {  // atlas.frag:284-295
    float u = f.u;
    if (om & F_SUBPIXEL) u -= r.aux * frcp(__builtin_fmaxf((float)atlas->size, 1.0f));
    const F4 t = atlas_sample(*atlas, u, f.v, f.lod);
    s.r = t.x * f.col.x; s.g = t.y * f.col.y; s.b = t.z * f.col.z; s.a = t.w * f.col.w;
    return s;
  }
  if (mode >= 13u && mode <= 16u) {  // atlas.frag:296-318
    const F4 fc = eval_fill_rec(r, f.col, fill_mode, f.u, f.v);
    const F4 t = atlas_sample(*atlas, f.u, f.v, 0.0f);  // textureLod(atlasTex, uv, 0.0)
    const bool is_mtsdf = (mode == 14u || mode == 16u), is_stroke = (mode == 15u || mode == 16u);
    const float sd = is_mtsdf ? t.w : median3(t.x, t.y, t.z);
    const float unit = r.f0 * frcp(r.p0);  // pxRange / atlas size (atlas.frag:45-49)
    const float spr = __builtin_fmaxf(0.5f * (unit * frcp(f.fw_u) + unit * frcp(f.fw_v)), 1.0f);
    const float spd = spr * (sd - r.f1);
    const float alpha = is_stroke ? clamp01(__builtin_fmaxf(r.p1, 0.0f) * 0.5f - __builtin_fabsf(spd) + 0.5f) : clamp01(spd + 0.5f);
    s.r = fc.x; s.g = fc.y; s.b = fc.z; s.a = fc.w * alpha;
    return s;
  }
  const float qhx = r.p0, qhy = r.p1;
  const bool inset = mode == 9u;
  const float shx = inset ? qhx : r.p2, shy = inset ? qhy : r.p3;
  const float lx = (f.u - 0.5f) * 2.0f * qhx, ly = (f.v - 0.5f) * 2.0f * qhy;
  const bool bezier = mode >= 18u && mode <= 20u;  // isBezierStrokeMode atlas.frag:162-168 (p is NOT y-flipped here)
  const float dist = bezier ? sd_bezier(lx, ly, r.p2, r.p3, r.r[0], r.r[1], r.r[2], r.r[3])
                            : shape_dist(ellip, lx, -ly, shx, shy, r.r[0], r.r[1], r.r[2], r.r[3]);
  const float spread = fill_mode == 0u ? r.f1 : 0.0f;
  float alpha;
  switch (mode) {
    case 18u: case 19u: case 20u: {  // atlas.frag:321-336
      const float sd = bezier_stroke_sd(dist, lx, ly, r.p2, r.p3, r.r[0], r.r[1], r.r[2], r.r[3], __builtin_fmaxf(r.f0, 0.0f) * 0.5f, mode);
      alpha = 1.0f - clamp01(r.aa * sd + 0.5f);
      break;
    }
    case 11u: { float h = r.f0 * 0.5f; float sd = __builtin_fabsf(dist + h) - h; alpha = sd < 0.0f ? 1.0f : 0.0f; break; }
    case 12u: { float h = r.f0 * 0.5f; float sd = __builtin_fabsf(dist + h) - h; alpha = 1.0f - clamp01(r.aa * sd + 0.5f); break; }
    case 7u: { float sd = dist - spread; const float sp = __builtin_fminf(shadow_profile(sd, r.f0), 1.0f); alpha = sd > 0.0f ? sp : 1.0f; break; }
    case 8u: {
      float inside = 1.0f - clamp01(r.aa * dist + 0.5f);
      float sd = dist - spread;
      const float sp = __builtin_fminf(shadow_profile(sd, r.f0), 1.0f);
      alpha = sd >= 0.0f ? sp : inside;
      break;
    }
    case 9u: {  // atlas.frag:364-380
      float clip_a = 1.0f - clamp01(r.aa * dist + 0.5f);
      float shd = shape_dist(ellip, lx - r.p2, -ly + r.p3, qhx, qhy, r.r[0], r.r[1], r.r[2], r.r[3]);
      float sd = shd + spread;
      const float sp = __builtin_fminf(shadow_profile(sd, r.f0), 1.0f);
      float ia = sd < 0.0f ? sp : 1.0f;
      alpha = clip_a * ia;
      break;
    }
    default: alpha = 1.0f - clamp01(r.aa * dist + 0.5f); break;
  }
  if (mode == 17u) {  // atlas.frag:381-388
    F4 b = F;
    if (!(om & F_SELF_BACKDROP) && in_frame) b = unpack255(backdrop[pix]);
    const float k = 1.0f / 255.0f;
    s.r = b.x * k; s.g = b.y * k; s.b = b.z * k; s.a = b.w * k * alpha;
  } else {
    const F4 fc = eval_fill_rec(r, f.col, fill_mode, f.u, f.v);
    s.r = fc.x; s.g = fc.y; s.b = fc.z; s.a = fc.w * alpha;
  }
  return s;
}

}  // namespace fdh
