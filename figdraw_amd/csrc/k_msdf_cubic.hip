// k_msdf_cubic.hip -- distance-field generation for outlines that hold cubic segments: fdh_put_glyph_outline_cubic with FDH_GLYPH_MTSDF (the
// specification is the comment in include_glyphs/figdraw_hip_cubic.h; this file is its steps 4 and 5).  k_msdf.hip's mapping and walk --
// a lane per texel, a wave per 8 x 8 tile, the edge index the loop counter so that records arrive by scalar loads, the per-tile cull, four
// running candidates, signs and pseudo-distances once after the loop -- over records of msdf::cubic::kCubicEdgeFloats floats
// (fdh_msdf_cubic_host.h) that hold lines, quadratics and cubics.  The kind is the record's: a scalar branch.  A line or a quadratic runs
// k_msdf.hip's statements (msdf_at, msdf_nearest_t, msdf_edge below are copies, kept in a namespace of their own: tests hold k_msdf.hip
// alone under their shims, so it shares no header), which gives such an edge of a mixed outline the bits it has there.  A cubic's nearest
// parameter has no closed form: cubic_nearest_t searches for it.
#include "fdh_device.h"
#include "fdh_msdf_cubic_host.h"

namespace fdh {
namespace cubic {

#ifndef FDH_MSDF_NO_CULL
#define FDH_MSDF_NO_CULL 0  // the tests' second build: every tile walks every edge
#endif
constexpr int kRec = msdf::cubic::kCubicEdgeFloats;

// ------------------------------------------------------------------ lines and quadratics: k_msdf.hip's, statement for statement
__device__ __forceinline__ void msdf_at(const float* __restrict__ r, float t, float px, float py, float& Ex, float& Ey, float& Tx, float& Ty) {
#pragma clang fp contract(off)
  const float dx = r[0] - px, dy = r[1] - py;
  float ex, ey;
  if (r[7] == 0.0f) {  // a line: P0 + e t
    ex = dx + r[8] * t; ey = dy + r[9] * t;
    Tx = r[8]; Ty = r[9];
  } else {
    ex = dx + (2.0f * r[8] + r[10] * t) * t; ey = dy + (2.0f * r[9] + r[11] * t) * t;
    Tx = r[8] + r[10] * t; Ty = r[9] + r[11] * t;
  }
  const float e1x = r[4] - px, e1y = r[5] - py;
  Ex = t <= 0.0f ? dx : (t >= 1.0f ? e1x : ex);
  Ey = t <= 0.0f ? dy : (t >= 1.0f ? e1y : ey);
}
__device__ __forceinline__ float msdf_d2(const float* __restrict__ r, float t, float px, float py) {
  float Ex, Ey, Tx, Ty;
  msdf_at(r, t, px, py, Ex, Ey, Tx, Ty);
  return Ex * Ex + Ey * Ey;
}
__device__ __forceinline__ float msdf_nearest_t(const float* __restrict__ r, float px, float py) {
#pragma clang fp contract(off)
  const float dx = r[0] - px, dy = r[1] - py;
  if (r[7] == 0.0f) return clamp01(-(dx * r[8] + dy * r[9]) * r[12]);  // wave-uniform
  const float ax = r[8], ay = r[9], bx = r[10], by = r[11], kk = r[12], kx = r[13], aa2 = r[14];
  const float ky = kk * (aa2 + (dx * bx + dy * by)) / 3.0f;
  const float kz = kk * (dx * ax + dy * ay);
  const float p = ky - kx * kx;
  const float p3 = p * p * p;
  const float q = kx * (2.0f * kx * kx - 3.0f * ky) + kz;
  const float h = q * q + 4.0f * p3;
  // h >= 0: one real root
  const float hs = __builtin_sqrtf(__builtin_fmaxf(h, 0.0f));
  const float tA = cbrt_signed((hs - q) * 0.5f) + cbrt_signed((-hs - q) * 0.5f) - kx;
  // h < 0 (then p < 0): three, the outer two are minima
  const float z = __builtin_sqrtf(__builtin_fmaxf(-p, 0.0f));
  const float den = p * z * 2.0f;
  const float arg = __builtin_fminf(__builtin_fmaxf(q / (den == 0.0f ? 1.0f : den), -1.0f), 1.0f);
  const float v = acos_poly(den == 0.0f ? 0.0f : arg) * (1.0f / 3.0f);
  const float v2 = v * v;
  float cm = -1.0f / 3628800.0f, sn = -1.0f / 39916800.0f;
  cm = __builtin_fmaf(cm, v2, 1.0f / 40320.0f); cm = __builtin_fmaf(cm, v2, -1.0f / 720.0f); cm = __builtin_fmaf(cm, v2, 1.0f / 24.0f); cm = __builtin_fmaf(cm, v2, -0.5f); cm = __builtin_fmaf(cm, v2, 1.0f);
  sn = __builtin_fmaf(sn, v2, 1.0f / 362880.0f); sn = __builtin_fmaf(sn, v2, -1.0f / 5040.0f); sn = __builtin_fmaf(sn, v2, 1.0f / 120.0f); sn = __builtin_fmaf(sn, v2, -1.0f / 6.0f); sn = __builtin_fmaf(sn, v2, 1.0f);
  const float m = cm, n = sn * v * 1.732050808f;
  const float t1 = (m + m) * z - kx, t2 = (-n - m) * z - kx;
  float best_t = 0.0f, best_d2 = 3.0e38f;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float t0 = h >= 0.0f ? tA : (k == 0 ? t1 : t2);
    float tn = t0;
#pragma unroll
    for (int it = 0; it < 2; it++) {
      const float Ex = dx + (2.0f * ax + bx * tn) * tn, Ey = dy + (2.0f * ay + by * tn) * tn;
      const float Tx = ax + bx * tn, Ty = ay + by * tn;
      const float g = Ex * Tx + Ey * Ty, gp = 2.0f * (Tx * Tx + Ty * Ty) + (Ex * bx + Ey * by);
      const float step = g * frcp(gp);
      tn = gp > 0.0f ? tn - step : tn;
    }
    const float ca = clamp01(t0), cb = clamp01(tn);
    const float da = msdf_d2(r, ca, px, py), db = msdf_d2(r, cb, px, py);
    const float tk = db < da ? cb : ca, dk = db < da ? db : da;
    if (dk < best_d2) { best_d2 = dk; best_t = tk; }
  }
  const float e1x = r[4] - px, e1y = r[5] - py;
  const float d0 = dx * dx + dy * dy, d1 = e1x * e1x + e1y * e1y;
  const float te = d1 < d0 ? 1.0f : 0.0f, de = d1 < d0 ? d1 : d0;
  return de <= best_d2 ? te : best_t;
}

// ------------------------------------------------------------------ cubics
// E(t) = B(t) - p, T(t) = B'(t) and g(t) = E . T of a cubic record in the power basis, Horner's form; dx, dy = P0 - p
#define FDH_CUBIC_EVAL(t)                                                                          \
  const float Ex = dx + ((r[12] * (t) + r[10]) * (t) + r[8]) * (t), Ey = dy + ((r[13] * (t) + r[11]) * (t) + r[9]) * (t); \
  const float Tx = (r[26] * (t) + r[24]) * (t) + r[8], Ty = (r[27] * (t) + r[25]) * (t) + r[9];   \
  const float g = Ex * Tx + Ey * Ty
// B(t) - p where a decision is taken on it: from the nearer end, so that close to an end the offset from that end keeps its own precision
// (a curve that halts at an end, P2 = P3, moves by less than a float32 step of its coordinates there: what then differs from the end point
// is rounding, and the texel would miss the end's pseudo-distance)
__device__ __forceinline__ void cubic_E(const float* __restrict__ r, float t, float px, float py, float& Ex, float& Ey) {
#pragma clang fp contract(off)
  const float s = 1.0f - t;
  const float fx = (r[0] - px) + ((r[12] * t + r[10]) * t + r[8]) * t, fy = (r[1] - py) + ((r[13] * t + r[11]) * t + r[9]) * t;
  const float bx = (r[4] - px) - ((r[12] * s - r[32]) * s + r[30]) * s, by = (r[5] - py) - ((r[13] * s - r[33]) * s + r[31]) * s;
  Ex = t <= 0.5f ? fx : bx; Ey = t <= 0.5f ? fy : by;
}
constexpr int kNewton = 6;
// kNewton steps of Newton on g from t inside [lo, hi].  bracketed: g(lo) < 0 <= g(hi) -- a minimum of the distance lies between --, every
// evaluation moves the end of its sign, and a step that leaves the bracket (or a g' that is not positive) is replaced by the bracket's middle.
// Otherwise: msdfgen's descent, a step taken where g' > 0 and held inside the window.  A fixed trip count, selects only.
template <bool bracketed>
__device__ __forceinline__ float cubic_refine(const float* __restrict__ r, float dx, float dy, float t, float lo, float hi) {
#pragma clang fp contract(off)
#pragma unroll
  for (int it = 0; it < kNewton; it++) {
    FDH_CUBIC_EVAL(t);
    const float Bx = 2.0f * r[26] * t + r[24], By = 2.0f * r[27] * t + r[25];  // B''(t)
    const float gp = (Tx * Tx + Ty * Ty) + (Ex * Bx + Ey * By);
    const float tn = t - g / (gp > 0.0f ? gp : 1.0f);
    if (bracketed) {
      lo = g < 0.0f ? t : lo; hi = g < 0.0f ? hi : t;
      t = (gp > 0.0f && tn > lo && tn < hi) ? tn : 0.5f * (lo + hi);
    } else {
      t = gp > 0.0f ? __builtin_fminf(__builtin_fmaxf(tn, lo), hi) : t;
    }
  }
  return t;
}
// The parameter of the point of the cubic r nearest to p: a root of the quintic g.  g is sampled at K + 1 uniform parameters (K: slot 14,
// chosen by the host from the curve's turning and its change of speed, wave-uniform); each interval over which g rises through zero
// holds a minimum of the distance -- a quintic has at most three --, and its bracket is refined; so is, without a bracket, the sample of
// smallest distance, which catches a maximum and a minimum inside one interval.  A candidate is kept only if B(t) itself came nearer.
// Then msdf_nearest_t's last rule: an interior point counts only where it is strictly nearer than both ends.
__device__ __forceinline__ float cubic_nearest_t(const float* __restrict__ r, float px, float py) {
#pragma clang fp contract(off)
  const float dx = r[0] - px, dy = r[1] - py;
  const int K = (int)r[14];
  const float step = 1.0f / (float)K;
  float g_prev = dx * r[8] + dy * r[9], t_prev = 0.0f;
  float best_t = 0.0f, best_d2 = dx * dx + dy * dy;
  float lo0 = -1.0f, lo1 = -1.0f, lo2 = -1.0f;
  for (int j = 1; j <= K; j++) {  // wave-uniform
    const float t = j == K ? 1.0f : (float)j * step;
    FDH_CUBIC_EVAL(t);
    const float d2 = Ex * Ex + Ey * Ey;
    const bool rise = g_prev < 0.0f && g >= 0.0f;
    const bool to2 = rise && lo1 >= 0.0f && lo2 < 0.0f, to1 = rise && lo0 >= 0.0f && lo1 < 0.0f, to0 = rise && lo0 < 0.0f;
    lo2 = to2 ? t_prev : lo2; lo1 = to1 ? t_prev : lo1; lo0 = to0 ? t_prev : lo0;
    const bool nearer = d2 < best_d2;
    best_t = nearer ? t : best_t; best_d2 = nearer ? d2 : best_d2;
    g_prev = g; t_prev = t;
  }
  const float seed_t = best_t;
  {
    float Ex, Ey;
    cubic_E(r, seed_t, px, py, Ex, Ey);
    best_d2 = Ex * Ex + Ey * Ey;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float lo = k == 0 ? lo0 : (k == 1 ? lo1 : lo2);
    float t;
    if (k == 3) {
      t = cubic_refine<false>(r, dx, dy, seed_t, __builtin_fmaxf(seed_t - step, 0.0f), __builtin_fminf(seed_t + step, 1.0f));
    } else {
      if (!(lo >= 0.0f)) continue;  // (a lane without this bracket: nothing to refine; most texels have one)
      const float hi = __builtin_fminf(lo + step, 1.0f);
      t = cubic_refine<true>(r, dx, dy, 0.5f * (lo + hi), lo, hi);
    }
    float Ex, Ey;
    cubic_E(r, t, px, py, Ex, Ey);
    const float d2 = Ex * Ex + Ey * Ey;
    const bool nearer = d2 < best_d2;
    best_t = nearer ? t : best_t; best_d2 = nearer ? d2 : best_d2;
  }
  const float e1x = r[4] - px, e1y = r[5] - py;
  const float d0 = dx * dx + dy * dy, d1 = e1x * e1x + e1y * e1y;
  const float te = d1 < d0 ? 1.0f : 0.0f, de = d1 < d0 ? d1 : d0;
  return de <= best_d2 ? te : best_t;
}
// msdf_at for a cubic: at t = 0 and t = 1 the stored end point and the stored unit tangent of that end (where a control point lies on
// the end, B' is zero there and the tangent is the next difference that is not)
__device__ __forceinline__ void cubic_at(const float* __restrict__ r, float t, float px, float py, float& Ex_, float& Ey_, float& Tx_, float& Ty_) {
#pragma clang fp contract(off)
  const float dx = r[0] - px, dy = r[1] - py;
  float Ex, Ey;
  cubic_E(r, t, px, py, Ex, Ey);
  const float Tx = (r[26] * t + r[24]) * t + r[8], Ty = (r[27] * t + r[25]) * t + r[9];
  const float e1x = r[4] - px, e1y = r[5] - py;
  Ex_ = t <= 0.0f ? dx : (t >= 1.0f ? e1x : Ex);
  Ey_ = t <= 0.0f ? dy : (t >= 1.0f ? e1y : Ey);
  Tx_ = t <= 0.0f ? r[16] : (t >= 1.0f ? r[18] : Tx);
  Ty_ = t <= 0.0f ? r[17] : (t >= 1.0f ? r[19] : Ty);
}
#undef FDH_CUBIC_EVAL

// ------------------------------------------------------------------ any edge: the kind is the record's, wave-uniform
__device__ __forceinline__ void edge_at(const float* __restrict__ r, float t, float px, float py, float& Ex, float& Ey, float& Tx, float& Ty) {
  if (r[7] == 2.0f) cubic_at(r, t, px, py, Ex, Ey, Tx, Ty);
  else msdf_at(r, t, px, py, Ex, Ey, Tx, Ty);
}
// what one edge offers a point p (k_msdf.hip's msdf_edge): the parameter of its nearest point, the squared distance, the orthogonality
// there and side = cross(T, p - N)
__device__ __forceinline__ void edge_offer(const float* __restrict__ r, float px, float py, float& t, float& d2, float& ortho, float& side) {
#pragma clang fp contract(off)
  t = r[7] == 2.0f ? cubic_nearest_t(r, px, py) : msdf_nearest_t(r, px, py);
  float Ex, Ey, Tx, Ty;
  edge_at(r, t, px, py, Ex, Ey, Tx, Ty);
  d2 = Ex * Ex + Ey * Ey;
  // orthogonality: |cross(unit tangent, unit vector to the texel)|; 0 on the curve itself, and at a cusp (T = 0)
  const float cr = Tx * Ey - Ty * Ex, den = (Tx * Tx + Ty * Ty) * d2;
  ortho = den > 0.0f ? __builtin_fabsf(cr) * frcp(fsqrt(den)) : 0.0f;
  side = Ty * Ex - Tx * Ey;  // the vector to the point is -E
}

// k_msdf_generate over the wider records
__global__ __launch_bounds__(64) void k_msdf_generate_cubic(const float* __restrict__ edges, int n_edges, int w, int h, float orient, float inv_range,
                                                            uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int tx0 = blockIdx.x * 8, ty0 = blockIdx.y * 8;
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  if (x >= w || y >= h) return;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#if !FDH_MSDF_NO_CULL
  // k_msdf_generate's cull: an end point bounds every carried channel from above, the control box (of all four points, for a cubic:
  // it holds the curve) bounds the edge from below
  constexpr float kHalfDiag = 4.9497475f + 1.0e-3f;
  const float mx = (float)tx0 + 4.0f, my = (float)ty0 + 4.0f;
  float ub[3] = {3.0e38f, 3.0e38f, 3.0e38f};
  for (int i = 0; i < n_edges; i++) {
    const float* __restrict__ r = edges + (size_t)i * kRec;
    const float ux = r[0] - mx, uy = r[1] - my, vx = r[4] - mx, vy = r[5] - my;
    const float u = fsqrt(__builtin_fminf(ux * ux + uy * uy, vx * vx + vy * vy)) + kHalfDiag;
    const int mask = (int)r[6];
#pragma unroll
    for (int c = 0; c < 3; c++) if ((mask >> c) & 1) ub[c] = __builtin_fminf(ub[c], u);
  }
#endif
  float bd2[4], bo[4], bt[4];
  int be[4];
#pragma unroll
  for (int c = 0; c < 4; c++) { bd2[c] = 3.0e38f; bo[c] = -1.0f; bt[c] = 0.0f; be[c] = -1; }
  for (int i = 0; i < n_edges; i++) {
    const float* __restrict__ r = edges + (size_t)i * kRec;
    const int mask = (int)r[6];
#if !FDH_MSDF_NO_CULL
    {
      const float gx = __builtin_fmaxf(__builtin_fmaxf(r[20] - mx, mx - r[22]), 0.0f), gy = __builtin_fmaxf(__builtin_fmaxf(r[21] - my, my - r[23]), 0.0f);
      const float lb = fsqrt(gx * gx + gy * gy) - kHalfDiag;
      float um = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; c++) if ((mask >> c) & 1) um = __builtin_fmaxf(um, ub[c]);
      if (lb > um * 1.0001f) continue;  // wave-uniform
    }
#endif
    float t, d2, ortho, side;
    edge_offer(r, px, py, t, d2, ortho, side);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (c < 3 && !((mask >> c) & 1)) continue;  // wave-uniform
      const bool better = d2 < bd2[c] || (d2 == bd2[c] && ortho > bo[c]);
      bd2[c] = better ? d2 : bd2[c]; bo[c] = better ? ortho : bo[c]; bt[c] = better ? t : bt[c]; be[c] = better ? i : be[c];
    }
  }
  uint32_t word = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    float d = -3.0e38f;  // no edge: outside
    if (be[c] >= 0) {
      const float* __restrict__ r = edges + (size_t)be[c] * kRec;
      float Ex, Ey, Tx, Ty;
      edge_at(r, bt[c], px, py, Ex, Ey, Tx, Ty);
      // the vector to the texel is -E: cross(T, p - N) = Ty Ex - Tx Ey
      const float cr = Ty * Ex - Tx * Ey;
      d = fsqrt(bd2[c]);
      d = cr >= 0.0f ? d : -d;
      if (c < 3 && (bt[c] <= 0.0f || bt[c] >= 1.0f)) {  // the nearest point is an end: the distance to the tangent line there
        const float ux = bt[c] <= 0.0f ? r[16] : r[18], uy = bt[c] <= 0.0f ? r[17] : r[19];
        const float pd = uy * Ex - ux * Ey;
        d = __builtin_fabsf(pd) <= __builtin_fabsf(d) ? pd : d;
      }
      d *= orient;
    }
    const float v = clamp01(0.5f + d * inv_range);
    word |= (uint32_t)__builtin_floorf(255.0f * v + 0.5f) << (8 * c);
  }
  out[(size_t)y * w + x] = word;
}

// ------------------------------------------------------------------ step 5: k_msdf_correct over the wider records
__device__ __forceinline__ int msdf_ch(uint32_t v, int k) { return (int)((v >> (8 * k)) & 255u); }
__device__ __forceinline__ int msdf_median(int a, int b, int c) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int m = hi < c ? hi : c;
  return lo > m ? lo : m;
}
__device__ __forceinline__ int msdf_median(uint32_t v) { return msdf_median(msdf_ch(v, 0), msdf_ch(v, 1), msdf_ch(v, 2)); }
__device__ __forceinline__ int msdf_depth(uint32_t v) { const int e = 2 * msdf_median(v) - 255; return e < 0 ? -e : e; }
__device__ __forceinline__ bool msdf_candidate(uint32_t a, uint32_t b, int cp, int& N, int& D, bool& inside) {
  const int i = cp == 1 ? 1 : 0, j = cp == 0 ? 1 : 2;
  N = msdf_ch(a, i) - msdf_ch(a, j);
  D = N - (msdf_ch(b, i) - msdf_ch(b, j));
  if (D < 0) { N = -N; D = -D; }
  int V[3];
#pragma unroll
  for (int k = 0; k < 3; k++) V[k] = msdf_ch(a, k) * D + N * (msdf_ch(b, k) - msdf_ch(a, k));  // D times channel k at the crossing
  const int X = msdf_median(V[0], V[1], V[2]), ma = msdf_median(a), mb = msdf_median(b);
  inside = 2 * X > 255 * D;
  const bool outside = 2 * X < 255 * D;
  const bool crosses = (D > 0) & (N > 0) & (N < D);
  return crosses & (((2 * ma > 255) & (2 * mb > 255) & outside) | ((2 * ma < 255) & (2 * mb < 255) & inside));
}

// the one cross-lane operation: does any lane of the wave say yes?  (k_msdf.hip's; a host build that emulates the wave brings its own)
#ifndef FDH_MSDF_ANY
#ifdef __HIP__
#define FDH_MSDF_ANY(p) (__ballot(p) != 0)
#else
#define FDH_MSDF_ANY(p) (p)
#endif
#endif

// k_msdf_correct's two phases: integer candidates, then, for as long as any lane of the wave holds one, a walk of all edges without
// culling for the true distance at the candidate's point.  Lanes outside the image carry no candidate but stay until the last ballot.
__global__ __launch_bounds__(64) void k_msdf_correct_cubic(const float* __restrict__ edges, int n_edges, int w, int h, float orient, float step,
                                                           const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 8 + (threadIdx.x & 7), y = blockIdx.y * 8 + (threadIdx.x >> 3);
  const bool live = x < w && y < h;
  const int cx = x < w ? x : w - 1, cy = y < h ? y : h - 1;  // what is loaded lies inside the image whatever the lane
  const int xl = cx > 0 ? cx - 1 : 0, xr = cx + 1 < w ? cx + 1 : w - 1, yu = cy > 0 ? cy - 1 : 0, yd = cy + 1 < h ? cy + 1 : h - 1;
  const uint32_t c = in[(size_t)cy * w + cx];
  const uint32_t nb[4] = {in[(size_t)cy * w + xl], in[(size_t)cy * w + xr], in[(size_t)yu * w + cx], in[(size_t)yd * w + cx]};
  const bool has[4] = {live && x > 0, live && x + 1 < w, live && y > 0, live && y + 1 < h};
  uint32_t todo = 0;
#pragma unroll
  for (int p = 0; p < 4; p++) {
#pragma unroll
    for (int cp = 0; cp < 3; cp++) {
      int N, D;
      bool inside;
      const bool cand = msdf_candidate((p & 1) ? c : nb[p], (p & 1) ? nb[p] : c, cp, N, D, inside);
      todo |= (uint32_t)(cand & has[p] & (n_edges > 0)) << (3 * p + cp);
    }
  }
  const int depth = msdf_depth(c);
  bool mark = false;
  while (FDH_MSDF_ANY(todo != 0)) {  // wave-uniform
    const int bit = todo ? __builtin_ctz(todo) : 0, p = bit / 3, cp = bit - 3 * p;
    const uint32_t other = p == 0 ? nb[0] : (p == 1 ? nb[1] : (p == 2 ? nb[2] : nb[3]));
    int N, D;
    bool inside;
    const bool cand = msdf_candidate((p & 1) ? c : other, (p & 1) ? other : c, cp, N, D, inside) & (todo != 0);
    const float t = cand ? (float)N / (float)D : 0.0f;
    const float ax = (float)(x - (p == 0 ? 1 : 0)) + 0.5f, ay = (float)(y - (p == 2 ? 1 : 0)) + 0.5f;
    const float qx = p < 2 ? ax + t : ax, qy = p < 2 ? ay : ay + t;
    float bd2 = 3.0e38f, bo = -1.0f, bs = 0.0f;
    for (int i = 0; i < n_edges; i++) {
      const float* __restrict__ r = edges + (size_t)i * kRec;
      float te, d2, ortho, side;
      edge_offer(r, qx, qy, te, d2, ortho, side);
      const bool better = d2 < bd2 || (d2 == bd2 && ortho > bo);
      bd2 = better ? d2 : bd2; bo = better ? ortho : bo; bs = better ? side : bs;
    }
    float d = fsqrt(bd2);
    d = (bs >= 0.0f ? d : -d) * orient;
    // a point within one quantisation step of the outline convicts nobody
    const bool artefact = cand && (inside ? d < -step : d > step);
    mark = mark | (artefact & (depth >= msdf_depth(other)));
    todo &= todo - 1u;
  }
  if (live) out[(size_t)y * w + x] = mark ? ((c & 0xFF000000u) | (uint32_t)msdf_median(c) * 0x010101u) : c;
}

// ------------------------------------------------------------------ the two kernel bodies as functions of the tile origin
// k_msdf_generate_cubic and k_msdf_correct_cubic once more, statement for statement, with the tile's origin (tx0, ty0) a parameter where the
// kernels take it from blockIdx: what the batched kernels below run on one glyph's slice of a concatenated buffer (k_msdf.hip's pattern,
// for its reason: the kernels above do not call these, so they keep their instruction streams -- profiles/msdf.txt sections 6 and 8).
// tests/msdf_cubic_batch_emu holds the two forms to the same bytes, glyph by glyph.
__device__ __forceinline__ void cubic_generate_tile(const float* edges, int n_edges, int w, int h, float orient, float inv_range, uint32_t* out, int tx0, int ty0) {
#pragma clang fp contract(off)
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  if (x >= w || y >= h) return;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#if !FDH_MSDF_NO_CULL
  // k_msdf_generate's cull: an end point bounds every carried channel from above, the control box (of all four points, for a cubic:
  // it holds the curve) bounds the edge from below
  constexpr float kHalfDiag = 4.9497475f + 1.0e-3f;
  const float mx = (float)tx0 + 4.0f, my = (float)ty0 + 4.0f;
  float ub[3] = {3.0e38f, 3.0e38f, 3.0e38f};
  for (int i = 0; i < n_edges; i++) {
    const float* __restrict__ r = edges + (size_t)i * kRec;
    const float ux = r[0] - mx, uy = r[1] - my, vx = r[4] - mx, vy = r[5] - my;
    const float u = fsqrt(__builtin_fminf(ux * ux + uy * uy, vx * vx + vy * vy)) + kHalfDiag;
    const int mask = (int)r[6];
#pragma unroll
    for (int c = 0; c < 3; c++) if ((mask >> c) & 1) ub[c] = __builtin_fminf(ub[c], u);
  }
#endif
  float bd2[4], bo[4], bt[4];
  int be[4];
#pragma unroll
  for (int c = 0; c < 4; c++) { bd2[c] = 3.0e38f; bo[c] = -1.0f; bt[c] = 0.0f; be[c] = -1; }
  for (int i = 0; i < n_edges; i++) {
    const float* __restrict__ r = edges + (size_t)i * kRec;
    const int mask = (int)r[6];
#if !FDH_MSDF_NO_CULL
    {
      const float gx = __builtin_fmaxf(__builtin_fmaxf(r[20] - mx, mx - r[22]), 0.0f), gy = __builtin_fmaxf(__builtin_fmaxf(r[21] - my, my - r[23]), 0.0f);
      const float lb = fsqrt(gx * gx + gy * gy) - kHalfDiag;
      float um = 0.0f;
#pragma unroll
      for (int c = 0; c < 3; c++) if ((mask >> c) & 1) um = __builtin_fmaxf(um, ub[c]);
      if (lb > um * 1.0001f) continue;  // wave-uniform
    }
#endif
    float t, d2, ortho, side;
    edge_offer(r, px, py, t, d2, ortho, side);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      if (c < 3 && !((mask >> c) & 1)) continue;  // wave-uniform
      const bool better = d2 < bd2[c] || (d2 == bd2[c] && ortho > bo[c]);
      bd2[c] = better ? d2 : bd2[c]; bo[c] = better ? ortho : bo[c]; bt[c] = better ? t : bt[c]; be[c] = better ? i : be[c];
    }
  }
  uint32_t word = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    float d = -3.0e38f;  // no edge: outside
    if (be[c] >= 0) {
      const float* __restrict__ r = edges + (size_t)be[c] * kRec;
      float Ex, Ey, Tx, Ty;
      edge_at(r, bt[c], px, py, Ex, Ey, Tx, Ty);
      // the vector to the texel is -E: cross(T, p - N) = Ty Ex - Tx Ey
      const float cr = Ty * Ex - Tx * Ey;
      d = fsqrt(bd2[c]);
      d = cr >= 0.0f ? d : -d;
      if (c < 3 && (bt[c] <= 0.0f || bt[c] >= 1.0f)) {  // the nearest point is an end: the distance to the tangent line there
        const float ux = bt[c] <= 0.0f ? r[16] : r[18], uy = bt[c] <= 0.0f ? r[17] : r[19];
        const float pd = uy * Ex - ux * Ey;
        d = __builtin_fabsf(pd) <= __builtin_fabsf(d) ? pd : d;
      }
      d *= orient;
    }
    const float v = clamp01(0.5f + d * inv_range);
    word |= (uint32_t)__builtin_floorf(255.0f * v + 0.5f) << (8 * c);
  }
  out[(size_t)y * w + x] = word;
}
__device__ __forceinline__ void cubic_correct_tile(const float* edges, int n_edges, int w, int h, float orient, float step, const uint32_t* in, uint32_t* out,
                                                   int tx0, int ty0) {
#pragma clang fp contract(off)
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  const bool live = x < w && y < h;
  const int cx = x < w ? x : w - 1, cy = y < h ? y : h - 1;  // what is loaded lies inside the image whatever the lane
  const int xl = cx > 0 ? cx - 1 : 0, xr = cx + 1 < w ? cx + 1 : w - 1, yu = cy > 0 ? cy - 1 : 0, yd = cy + 1 < h ? cy + 1 : h - 1;
  const uint32_t c = in[(size_t)cy * w + cx];
  const uint32_t nb[4] = {in[(size_t)cy * w + xl], in[(size_t)cy * w + xr], in[(size_t)yu * w + cx], in[(size_t)yd * w + cx]};
  const bool has[4] = {live && x > 0, live && x + 1 < w, live && y > 0, live && y + 1 < h};
  uint32_t todo = 0;
#pragma unroll
  for (int p = 0; p < 4; p++) {
#pragma unroll
    for (int cp = 0; cp < 3; cp++) {
      int N, D;
      bool inside;
      const bool cand = msdf_candidate((p & 1) ? c : nb[p], (p & 1) ? nb[p] : c, cp, N, D, inside);
      todo |= (uint32_t)(cand & has[p] & (n_edges > 0)) << (3 * p + cp);
    }
  }
  const int depth = msdf_depth(c);
  bool mark = false;
  while (FDH_MSDF_ANY(todo != 0)) {  // wave-uniform
    const int bit = todo ? __builtin_ctz(todo) : 0, p = bit / 3, cp = bit - 3 * p;
    const uint32_t other = p == 0 ? nb[0] : (p == 1 ? nb[1] : (p == 2 ? nb[2] : nb[3]));
    int N, D;
    bool inside;
    const bool cand = msdf_candidate((p & 1) ? c : other, (p & 1) ? other : c, cp, N, D, inside) & (todo != 0);
    const float t = cand ? (float)N / (float)D : 0.0f;
    const float ax = (float)(x - (p == 0 ? 1 : 0)) + 0.5f, ay = (float)(y - (p == 2 ? 1 : 0)) + 0.5f;
    const float qx = p < 2 ? ax + t : ax, qy = p < 2 ? ay : ay + t;
    float bd2 = 3.0e38f, bo = -1.0f, bs = 0.0f;
    for (int i = 0; i < n_edges; i++) {
      const float* __restrict__ r = edges + (size_t)i * kRec;
      float te, d2, ortho, side;
      edge_offer(r, qx, qy, te, d2, ortho, side);
      const bool better = d2 < bd2 || (d2 == bd2 && ortho > bo);
      bd2 = better ? d2 : bd2; bo = better ? ortho : bo; bs = better ? side : bs;
    }
    float d = fsqrt(bd2);
    d = (bs >= 0.0f ? d : -d) * orient;
    // a point within one quantisation step of the outline convicts nobody
    const bool artefact = cand && (inside ? d < -step : d > step);
    mark = mark | (artefact & (depth >= msdf_depth(other)));
    todo &= todo - 1u;
  }
  if (live) out[(size_t)y * w + x] = mark ? ((c & 0xFF000000u) | (uint32_t)msdf_median(c) * 0x010101u) : c;
}

// ------------------------------------------------------------------ fdh_put_glyph_outlines_cubic: a batch of fields in one launch
// (the specification: include_glyphs/figdraw_hip_cubic_batch.h).  k_msdf_generate_batch and k_msdf_correct_batch of k_msdf.hip over the wider records:
// a 1-D grid over all 8 x 8 tiles of all glyphs, the tile's glyph (tile_glyph) and the glyph's record (msdf::BatchGlyph, fdh_msdf_host.h;
// edge_off counts records of kRec floats) read from blockIdx alone -- scalar loads, as the edge records behind them.  A tile lies inside
// its glyph's tile grid, so a store goes to the glyph's own w x h texels and nowhere else.  A glyph without a cubic has records of lines
// and quadratics only and runs k_msdf.hip's statements on them: its bytes are k_msdf_generate's and k_msdf_correct's.
#define FDH_CUBIC_BATCH_TILE                                                                     \
  const msdf::BatchGlyph g = glyphs[tile_glyph[blockIdx.x]];                                     \
  const int tile = (int)(blockIdx.x - g.first_tile), tiles_x = (g.w + 7) / 8;                    \
  const int ty0 = tile / tiles_x * 8, tx0 = (tile - tile / tiles_x * tiles_x) * 8;               \
  const float* __restrict__ rec = edges + (size_t)g.edge_off * kRec
__global__ __launch_bounds__(64) void k_msdf_generate_cubic_batch(const float* __restrict__ edges, const msdf::BatchGlyph* __restrict__ glyphs,
                                                                  const uint32_t* __restrict__ tile_glyph, uint32_t* __restrict__ out) {
  FDH_CUBIC_BATCH_TILE;
  cubic_generate_tile(rec, g.n_edges, g.w, g.h, g.orient, g.inv_range, out + g.field_off, tx0, ty0);
}
__global__ __launch_bounds__(64) void k_msdf_correct_cubic_batch(const float* __restrict__ edges, const msdf::BatchGlyph* __restrict__ glyphs,
                                                                 const uint32_t* __restrict__ tile_glyph, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  FDH_CUBIC_BATCH_TILE;
  cubic_correct_tile(rec, g.n_edges, g.w, g.h, g.orient, g.step, in + g.field_off, out + g.field_off, tx0, ty0);
}
#undef FDH_CUBIC_BATCH_TILE

}  // namespace cubic

void launch_msdf_generate_cubic(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, uint32_t* out) {
  if (w <= 0 || h <= 0) return;
  FDH_LAUNCH(cubic::k_msdf_generate_cubic, dim3((w + 7) / 8, (h + 7) / 8), dim3(64), 0, s, edges, n_edges, w, h, orient, 1.0f / range, out);
}
void launch_msdf_correct_cubic(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, const uint32_t* in, uint32_t* out) {
  if (w <= 0 || h <= 0) return;
  FDH_LAUNCH(cubic::k_msdf_correct_cubic, dim3((w + 7) / 8, (h + 7) / 8), dim3(64), 0, s, edges, n_edges, w, h, orient, range / 255.0f, in, out);
}
void launch_msdf_generate_cubic_batch(hipStream_t s, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, uint32_t* out) {
  if (n_tiles <= 0) return;
  FDH_LAUNCH(cubic::k_msdf_generate_cubic_batch, dim3(n_tiles), dim3(64), 0, s, edges, glyphs, tile_glyph, out);
}
void launch_msdf_correct_cubic_batch(hipStream_t s, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* in,
                                     uint32_t* out) {
  if (n_tiles <= 0) return;
  FDH_LAUNCH(cubic::k_msdf_correct_cubic_batch, dim3(n_tiles), dim3(64), 0, s, edges, glyphs, tile_glyph, in, out);
}

}  // namespace fdh
