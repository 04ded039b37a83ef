// k_msdf.hip -- distance-field generation: fdh_put_glyph_outline with FDH_GLYPH_MTSDF (the specification is the comment at that flag in
// include/figdraw_hip.h; this file is its step 4).  The host has split the outline into coloured edges (fdh_msdf_host.h); here one lane
// owns one texel, one wave an 8 x 8 tile of them, and walks every edge.  The edge records are wave-uniform -- their index is the loop
// counter -- so they arrive through scalar loads and what depends on the edge alone costs nothing per lane.  A lane keeps four running
// candidates (the channels R, G, B and the true distance): squared distance, orthogonality, edge and parameter; signs and
// pseudo-distances are made once, after the loop, from the winners.
// k_msdf_correct is step 5, the correction pass behind FDH_GLYPH_MTSDF_CORRECT: the same mapping over the quantised image; integers find the
// few places where interpolation between two texels carries the median across 0.5, and only a wave that holds one walks the edges again.
// k_msdf_generate_union and k_msdf_correct_union are step 6, FDH_GLYPH_MTSDF_OVERLAP: the same walk, taken contour by contour -- a contour's
// last record says so and whether it is filled or a hole --, each contour's result ranked into two lists of four, the texel's contour
// selected after the loop.
#include "fdh_device.h"
#include "fdh_msdf_host.h"

namespace fdh {

#ifndef FDH_MSDF_NO_CULL
#define FDH_MSDF_NO_CULL 0  // tools/msdf_bench.py's second build: every tile walks every edge
#endif

// E = B(t) - p and the tangent direction at t of edge r, t in [0, 1]; at t = 0 and t = 1 the point IS the stored end, so that the two
// edges that meet in a corner give a texel beyond it bit-identical distances (the tie the orthogonality then breaks)
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
// the parameter of the point of edge r nearest to p.  A quadratic: the closed-form solve of sd_bezierN (fdh_device.h) -- both cases
// evaluated, one selected -- which leaves a distance; here the parameter is the product, and it has to be good: the comparison is
// with a float64 reference, and the one-root case cancels (see the comment in sd_bezierN: IEEE division and square root, nothing
// contracted, up to the roots).  What the cancellation still costs is mended by two Newton steps on the geometric form
// g(t) = E(t) . T(t), whose rounding error does not grow with the cubic's coefficients; a step is kept only if it came nearer.
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
  // An interior point counts only where it is nearer than both ends.  Towards a control point that lies on its end point the curve slows
  // to a halt -- B(t) - P2 = (P0 - P2) (1 - t)^2 -- so a root 1e-6 short of 1 is the end itself to the last bit, and left at that the
  // texel would miss the end's pseudo-distance.
  const float e1x = r[4] - px, e1y = r[5] - py;
  const float d0 = dx * dx + dy * dy, d1 = e1x * e1x + e1y * e1y;
  const float te = d1 < d0 ? 1.0f : 0.0f, de = d1 < d0 ? d1 : d0;
  return de <= best_d2 ? te : best_t;
}

// what one edge offers a point p: the parameter of its nearest point, the squared distance, the orthogonality there and
// side = cross(T, p - N), whose sign is the side of the edge p lies on
__device__ __forceinline__ void msdf_edge(const float* __restrict__ r, float px, float py, float& t, float& d2, float& ortho, float& side) {
#pragma clang fp contract(off)
  t = msdf_nearest_t(r, px, py);
  float Ex, Ey, Tx, Ty;
  msdf_at(r, t, px, py, Ex, Ey, Tx, Ty);
  d2 = Ex * Ex + Ey * Ey;
  // orthogonality: |cross(unit tangent, unit vector to the texel)|; 0 on the curve itself
  const float cr = Tx * Ey - Ty * Ex, den = (Tx * Tx + Ty * Ty) * d2;
  ortho = den > 0.0f ? __builtin_fabsf(cr) * frcp(fsqrt(den)) : 0.0f;
  side = Ty * Ex - Tx * Ey;  // the vector to the point is -E
}

__global__ __launch_bounds__(64) void k_msdf_generate(const float* __restrict__ edges, int n_edges, int w, int h, float orient, float inv_range,
                                                      uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int tx0 = blockIdx.x * 8, ty0 = blockIdx.y * 8;
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  if (x >= w || y >= h) return;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#if !FDH_MSDF_NO_CULL
  // The tile's texel centres lie within kHalfDiag of its middle.  An end point of an edge at distance u from the middle is at most
  // u + kHalfDiag from every texel: an upper bound for each channel the edge carries.  An edge whose control box is farther than that from
  // every texel, for every channel it carries, cannot win anywhere in the tile (the true distance takes all edges: its bound is the
  // smallest of the three, so the largest bound among the carried channels decides).  Range culls nothing: a far texel's sign still
  // comes from its nearest edge.
  constexpr float kHalfDiag = 4.9497475f + 1.0e-3f;
  const float mx = (float)tx0 + 4.0f, my = (float)ty0 + 4.0f;
  float ub[3] = {3.0e38f, 3.0e38f, 3.0e38f};
  for (int i = 0; i < n_edges; i++) {
    const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
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
    const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
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
    msdf_edge(r, px, py, t, d2, ortho, side);
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
      const float* __restrict__ r = edges + (size_t)be[c] * msdf::kEdgeFloats;
      float Ex, Ey, Tx, Ty;
      msdf_at(r, bt[c], px, py, Ex, Ey, Tx, Ty);
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

void launch_msdf_generate(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, uint32_t* out) {
  if (w <= 0 || h <= 0) return;
  FDH_LAUNCH(k_msdf_generate, dim3((w + 7) / 8, (h + 7) / 8), dim3(64), 0, s, edges, n_edges, w, h, orient, 1.0f / range, out);
}

// ------------------------------------------------------------------ step 5 of the specification: the correction pass
__device__ __forceinline__ int msdf_ch(uint32_t v, int k) { return (int)((v >> (8 * k)) & 255u); }
__device__ __forceinline__ int msdf_median(int a, int b, int c) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int m = hi < c ? hi : c;
  return lo > m ? lo : m;
}
__device__ __forceinline__ int msdf_median(uint32_t v) { return msdf_median(msdf_ch(v, 0), msdf_ch(v, 1), msdf_ch(v, 2)); }
// how far a texel's median is from the outline's value 127.5, doubled
__device__ __forceinline__ int msdf_depth(uint32_t v) { const int e = 2 * msdf_median(v) - 255; return e < 0 ? -e : e; }
// The pair (a, b) of texels, a the left or upper one, and the channels (R, G), (G, B), (R, B) for cp = 0, 1, 2: do they cross between the two
// centres, and is that crossing a candidate -- both medians on one side of 127.5 and the interpolated one on the other?  Then it is at
// N / D of the way from a to b, and `inside` says on which side the interpolated median lies.  Integers only: whichever lane asks, and
// the reference, get the same answer.
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
  const bool crosses = (D > 0) & (N > 0) & (N < D);  // (&, |: a handful of compares, nothing to branch around)
  return crosses & (((2 * ma > 255) & (2 * mb > 255) & outside) | ((2 * ma < 255) & (2 * mb < 255) & inside));
}

// The one cross-lane operation of this file: does any lane of the wave say yes?  On the device a ballot.  A host build that emulates the
// 64 lanes of a wave together brings its own (tests/msdf_correct_emu); one that runs a lane at a time (tests/msdf_emu, which launches the
// generator only) has waves of one lane, and the lane's own word is the answer.
#ifndef FDH_MSDF_ANY
#ifdef __HIP__
#define FDH_MSDF_ANY(p) (__ballot(p) != 0)
#else
#define FDH_MSDF_ANY(p) (p)
#endif
#endif

// One lane per texel of the quantised image `in`, one wave per 8 x 8 tile, as in k_msdf_generate.  Phase 1: a lane looks at its four pairs
// (left, right, upper, lower neighbour; the neighbour may belong to another tile, `in` is only read) and notes the candidates in `todo`,
// bit 3 pair + channel pair.  Phase 2, for as long as any lane of the wave holds one: every lane takes its next candidate's point q -- always
// from the pair's left / upper texel, so that the two lanes of a pair ask about the bit-identical point and agree -- and the wave walks all
// edges once for the true distance there.  No culling: q needs every edge.  A convicted crossing marks this lane's texel when its median
// is at least as far from 127.5 as the other's; a marked texel leaves with R = G = B = median.  Lanes outside the image carry no
// candidate but stay until the last ballot.
__global__ __launch_bounds__(64) void k_msdf_correct(const float* __restrict__ edges, int n_edges, int w, int h, float orient, float step,
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
      const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
      float te, d2, ortho, side;
      msdf_edge(r, qx, qy, te, d2, ortho, side);
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

void launch_msdf_correct(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, const uint32_t* in, uint32_t* out) {
  if (w <= 0 || h <= 0) return;
  FDH_LAUNCH(k_msdf_correct, dim3((w + 7) / 8, (h + 7) / 8), dim3(64), 0, s, edges, n_edges, w, h, orient, range / 255.0f, in, out);
}

// ------------------------------------------------------------------ step 6 of the specification: overlapping contours
// Two ranked lists of at most four contours: the filled ones by A descending, the holes by A ascending; ties keep contour order (a strict
// compare finds the newcomer's place, so it never passes an equal earlier contour; what it displaces moves down without another compare, so
// no displaced entry passes its equal either).  T: what travels with A -- the texel's encoded word in the generator;
// the correction ranks A alone.  An absent filled entry is -3e38 (it never wins: an outline with edges has a filled contour), an absent
// hole +3e38 (min leaves the filled one).  All in registers: every index below is a constant after unrolling.
template <typename T> struct MsdfRank {
  float fa[4], ga[4];
  T fw[4], gw[4];
  __device__ __forceinline__ void clear(T none) {
#pragma unroll
    for (int k = 0; k < 4; k++) { fa[k] = -3.0e38f; ga[k] = 3.0e38f; fw[k] = none; gw[k] = none; }
  }
  // cls: slot 15 of the contour's last record (wave-uniform); negative: a hole
  __device__ __forceinline__ void insert(float cls, float a, T word) {
    if (!(cls < 0.0f)) {
      bool up = false;
#pragma unroll
      for (int k = 0; k < 4; k++) {  // the newcomer takes the first place whose holder it beats; from there on every entry moves down one
        up = up || a > fa[k];
        const float ta = fa[k]; const T tw = fw[k];
        fa[k] = up ? a : ta; fw[k] = up ? word : tw;
        a = up ? ta : a; word = up ? tw : word;
      }
    } else {
      bool up = false;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        up = up || a < ga[k];
        const float ta = ga[k]; const T tw = gw[k];
        ga[k] = up ? a : ta; gw[k] = up ? word : tw;
        a = up ? ta : a; word = up ? tw : word;
      }
    }
  }
  // the term f_k = min(a(F_k), a(G_k)) that is largest, ties to the lowest k -> its value, and the word of the contour it names
  __device__ __forceinline__ float select(T& word) const {
    float best = __builtin_fminf(fa[0], ga[0]);
    word = ga[0] < fa[0] ? gw[0] : fw[0];
#pragma unroll
    for (int k = 1; k < 4; k++) {
      const float f = __builtin_fminf(fa[k], ga[k]);
      const T wk = ga[k] < fa[k] ? gw[k] : fw[k];
      const bool up = f > best;
      word = up ? wk : word; best = up ? f : best;
    }
    return best;
  }
};

// k_msdf_generate's mapping and arithmetic, contour by contour: [first, last] is one contour (slot 15 of record `last` is not 0).  The cull
// is k_msdf_generate's with its bound taken among this contour's edges alone -- every contour carries every channel after step 3 -- so
// within a contour no edge that could win is skipped.  At the contour's end the tail that k_msdf_generate runs once makes the contour's
// four distances and their word; A and the word go into the ranking.  The walk over the records is bounded by n_edges whatever slot 15 holds.
__global__ __launch_bounds__(64) void k_msdf_generate_union(const float* __restrict__ edges, int n_edges, int w, int h, float orient, float inv_range,
                                                            uint32_t* __restrict__ out) {
#pragma clang fp contract(off)
  const int tx0 = blockIdx.x * 8, ty0 = blockIdx.y * 8;
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  if (x >= w || y >= h) return;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#if !FDH_MSDF_NO_CULL
  constexpr float kHalfDiag = 4.9497475f + 1.0e-3f;
  const float mx = (float)tx0 + 4.0f, my = (float)ty0 + 4.0f;
#endif
  MsdfRank<uint32_t> rank;
  rank.clear(0u);
  int first = 0;
  while (first < n_edges) {  // wave-uniform
    int last = first;
#if !FDH_MSDF_NO_CULL
    float ub[3] = {3.0e38f, 3.0e38f, 3.0e38f};
    for (;; last++) {  // the bound pass finds the contour's end as it goes
      const float* __restrict__ r = edges + (size_t)last * msdf::kEdgeFloats;
      const float ux = r[0] - mx, uy = r[1] - my, vx = r[4] - mx, vy = r[5] - my;
      const float u = fsqrt(__builtin_fminf(ux * ux + uy * uy, vx * vx + vy * vy)) + kHalfDiag;
      const int mask = (int)r[6];
#pragma unroll
      for (int c = 0; c < 3; c++) if ((mask >> c) & 1) ub[c] = __builtin_fminf(ub[c], u);
      if (r[15] != 0.0f || last + 1 >= n_edges) break;
    }
#else
    while (last + 1 < n_edges && edges[(size_t)last * msdf::kEdgeFloats + 15] == 0.0f) last++;
#endif
    float bd2[4], bo[4], bt[4];
    int be[4];
#pragma unroll
    for (int c = 0; c < 4; c++) { bd2[c] = 3.0e38f; bo[c] = -1.0f; bt[c] = 0.0f; be[c] = -1; }
    for (int i = first; i <= last; i++) {
      const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
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
      msdf_edge(r, px, py, t, d2, ortho, side);
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if (c < 3 && !((mask >> c) & 1)) continue;  // wave-uniform
        const bool better = d2 < bd2[c] || (d2 == bd2[c] && ortho > bo[c]);
        bd2[c] = better ? d2 : bd2[c]; bo[c] = better ? ortho : bo[c]; bt[c] = better ? t : bt[c]; be[c] = better ? i : be[c];
      }
    }
    uint32_t word = 0;
    float a = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float d = -3.0e38f;
      if (be[c] >= 0) {
        const float* __restrict__ r = edges + (size_t)be[c] * msdf::kEdgeFloats;
        float Ex, Ey, Tx, Ty;
        msdf_at(r, bt[c], px, py, Ex, Ey, Tx, Ty);
        const float cr = Ty * Ex - Tx * Ey;
        d = fsqrt(bd2[c]);
        d = cr >= 0.0f ? d : -d;
        if (c < 3 && (bt[c] <= 0.0f || bt[c] >= 1.0f)) {
          const float ux = bt[c] <= 0.0f ? r[16] : r[18], uy = bt[c] <= 0.0f ? r[17] : r[19];
          const float pd = uy * Ex - ux * Ey;
          d = __builtin_fabsf(pd) <= __builtin_fabsf(d) ? pd : d;
        }
        d *= orient;
      }
      if (c == 3) a = d;
      const float v = clamp01(0.5f + d * inv_range);
      word |= (uint32_t)__builtin_floorf(255.0f * v + 0.5f) << (8 * c);
    }
    rank.insert(edges[(size_t)last * msdf::kEdgeFloats + 15], a, word);
    first = last + 1;
  }
  uint32_t word;
  rank.select(word);
  out[(size_t)y * w + x] = word;
}

void launch_msdf_generate_union(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, uint32_t* out) {
  if (w <= 0 || h <= 0) return;
  FDH_LAUNCH(k_msdf_generate_union, dim3((w + 7) / 8, (h + 7) / 8), dim3(64), 0, s, edges, n_edges, w, h, orient, 1.0f / range, out);
}

// k_msdf_correct with step 6's verdict distance: phases as there, but phase 2's walk keeps (d2, ortho, side) per contour, makes the contour's
// true distance at its end and ranks that scalar; d(q) is the largest term.
__global__ __launch_bounds__(64) void k_msdf_correct_union(const float* __restrict__ edges, int n_edges, int w, int h, float orient, float step,
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
    MsdfRank<uint32_t> rank;  // (the words are never read here: the compiler drops them)
    rank.clear(0u);
    float bd2 = 3.0e38f, bo = -1.0f, bs = 0.0f;
    for (int i = 0; i < n_edges; i++) {
      const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
      float te, d2, ortho, side;
      msdf_edge(r, qx, qy, te, d2, ortho, side);
      const bool better = d2 < bd2 || (d2 == bd2 && ortho > bo);
      bd2 = better ? d2 : bd2; bo = better ? ortho : bo; bs = better ? side : bs;
      if (r[15] != 0.0f || i + 1 == n_edges) {  // wave-uniform: the contour ends here
        const float dc = fsqrt(bd2);
        rank.insert(r[15], (bs >= 0.0f ? dc : -dc) * orient, 0u);
        bd2 = 3.0e38f; bo = -1.0f; bs = 0.0f;
      }
    }
    uint32_t none;
    const float d = rank.select(none);
    // a point within one quantisation step of the outline convicts nobody
    const bool artefact = cand && (inside ? d < -step : d > step);
    mark = mark | (artefact & (depth >= msdf_depth(other)));
    todo &= todo - 1u;
  }
  if (live) out[(size_t)y * w + x] = mark ? ((c & 0xFF000000u) | (uint32_t)msdf_median(c) * 0x010101u) : c;
}

void launch_msdf_correct_union(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, const uint32_t* in, uint32_t* out) {
  if (w <= 0 || h <= 0) return;
  FDH_LAUNCH(k_msdf_correct_union, dim3((w + 7) / 8, (h + 7) / 8), dim3(64), 0, s, edges, n_edges, w, h, orient, range / 255.0f, in, out);
}

// ------------------------------------------------------------------ the four kernel bodies as functions of the tile origin
// k_msdf_generate, k_msdf_correct, k_msdf_generate_union and k_msdf_correct_union once more, statement for statement, with the tile's origin
// (tx0, ty0) a parameter where the kernels take it from blockIdx: what the batched kernels below run on one glyph's slice of a
// concatenated buffer.  The kernels above do not call these: inlined into them the same statements compile to another instruction
// stream (profiles/msdf.txt section 6), and section 5 there keeps the single put's kernels instruction for instruction what they were.
// tests/msdf_batch_emu holds the two forms to the same bytes, glyph by glyph.
__device__ __forceinline__ void msdf_generate_tile(const float* edges, int n_edges, int w, int h, float orient, float inv_range,
                                                   uint32_t* out, int tx0, int ty0) {
#pragma clang fp contract(off)
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  if (x >= w || y >= h) return;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#if !FDH_MSDF_NO_CULL
  // The tile's texel centres lie within kHalfDiag of its middle.  An end point of an edge at distance u from the middle is at most
  // u + kHalfDiag from every texel: an upper bound for each channel the edge carries.  An edge whose control box is farther than that from
  // every texel, for every channel it carries, cannot win anywhere in the tile (the true distance takes all edges: its bound is the
  // smallest of the three, so the largest bound among the carried channels decides).  Range culls nothing: a far texel's sign still
  // comes from its nearest edge.
  constexpr float kHalfDiag = 4.9497475f + 1.0e-3f;
  const float mx = (float)tx0 + 4.0f, my = (float)ty0 + 4.0f;
  float ub[3] = {3.0e38f, 3.0e38f, 3.0e38f};
  for (int i = 0; i < n_edges; i++) {
    const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
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
    const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
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
    msdf_edge(r, px, py, t, d2, ortho, side);
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
      const float* __restrict__ r = edges + (size_t)be[c] * msdf::kEdgeFloats;
      float Ex, Ey, Tx, Ty;
      msdf_at(r, bt[c], px, py, Ex, Ey, Tx, Ty);
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
__device__ __forceinline__ void msdf_correct_tile(const float* edges, int n_edges, int w, int h, float orient, float step,
                                                  const uint32_t* in, uint32_t* out, int tx0, int ty0) {
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
      const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
      float te, d2, ortho, side;
      msdf_edge(r, qx, qy, te, d2, ortho, side);
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
__device__ __forceinline__ void msdf_generate_union_tile(const float* edges, int n_edges, int w, int h, float orient, float inv_range,
                                                         uint32_t* out, int tx0, int ty0) {
#pragma clang fp contract(off)
  const int x = tx0 + (threadIdx.x & 7), y = ty0 + (threadIdx.x >> 3);
  if (x >= w || y >= h) return;
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#if !FDH_MSDF_NO_CULL
  constexpr float kHalfDiag = 4.9497475f + 1.0e-3f;
  const float mx = (float)tx0 + 4.0f, my = (float)ty0 + 4.0f;
#endif
  MsdfRank<uint32_t> rank;
  rank.clear(0u);
  int first = 0;
  while (first < n_edges) {  // wave-uniform
    int last = first;
#if !FDH_MSDF_NO_CULL
    float ub[3] = {3.0e38f, 3.0e38f, 3.0e38f};
    for (;; last++) {  // the bound pass finds the contour's end as it goes
      const float* __restrict__ r = edges + (size_t)last * msdf::kEdgeFloats;
      const float ux = r[0] - mx, uy = r[1] - my, vx = r[4] - mx, vy = r[5] - my;
      const float u = fsqrt(__builtin_fminf(ux * ux + uy * uy, vx * vx + vy * vy)) + kHalfDiag;
      const int mask = (int)r[6];
#pragma unroll
      for (int c = 0; c < 3; c++) if ((mask >> c) & 1) ub[c] = __builtin_fminf(ub[c], u);
      if (r[15] != 0.0f || last + 1 >= n_edges) break;
    }
#else
    while (last + 1 < n_edges && edges[(size_t)last * msdf::kEdgeFloats + 15] == 0.0f) last++;
#endif
    float bd2[4], bo[4], bt[4];
    int be[4];
#pragma unroll
    for (int c = 0; c < 4; c++) { bd2[c] = 3.0e38f; bo[c] = -1.0f; bt[c] = 0.0f; be[c] = -1; }
    for (int i = first; i <= last; i++) {
      const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
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
      msdf_edge(r, px, py, t, d2, ortho, side);
#pragma unroll
      for (int c = 0; c < 4; c++) {
        if (c < 3 && !((mask >> c) & 1)) continue;  // wave-uniform
        const bool better = d2 < bd2[c] || (d2 == bd2[c] && ortho > bo[c]);
        bd2[c] = better ? d2 : bd2[c]; bo[c] = better ? ortho : bo[c]; bt[c] = better ? t : bt[c]; be[c] = better ? i : be[c];
      }
    }
    uint32_t word = 0;
    float a = -3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      float d = -3.0e38f;
      if (be[c] >= 0) {
        const float* __restrict__ r = edges + (size_t)be[c] * msdf::kEdgeFloats;
        float Ex, Ey, Tx, Ty;
        msdf_at(r, bt[c], px, py, Ex, Ey, Tx, Ty);
        const float cr = Ty * Ex - Tx * Ey;
        d = fsqrt(bd2[c]);
        d = cr >= 0.0f ? d : -d;
        if (c < 3 && (bt[c] <= 0.0f || bt[c] >= 1.0f)) {
          const float ux = bt[c] <= 0.0f ? r[16] : r[18], uy = bt[c] <= 0.0f ? r[17] : r[19];
          const float pd = uy * Ex - ux * Ey;
          d = __builtin_fabsf(pd) <= __builtin_fabsf(d) ? pd : d;
        }
        d *= orient;
      }
      if (c == 3) a = d;
      const float v = clamp01(0.5f + d * inv_range);
      word |= (uint32_t)__builtin_floorf(255.0f * v + 0.5f) << (8 * c);
    }
    rank.insert(edges[(size_t)last * msdf::kEdgeFloats + 15], a, word);
    first = last + 1;
  }
  uint32_t word;
  rank.select(word);
  out[(size_t)y * w + x] = word;
}
__device__ __forceinline__ void msdf_correct_union_tile(const float* edges, int n_edges, int w, int h, float orient, float step,
                                                        const uint32_t* in, uint32_t* out, int tx0, int ty0) {
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
    MsdfRank<uint32_t> rank;  // (the words are never read here: the compiler drops them)
    rank.clear(0u);
    float bd2 = 3.0e38f, bo = -1.0f, bs = 0.0f;
    for (int i = 0; i < n_edges; i++) {
      const float* __restrict__ r = edges + (size_t)i * msdf::kEdgeFloats;
      float te, d2, ortho, side;
      msdf_edge(r, qx, qy, te, d2, ortho, side);
      const bool better = d2 < bd2 || (d2 == bd2 && ortho > bo);
      bd2 = better ? d2 : bd2; bo = better ? ortho : bo; bs = better ? side : bs;
      if (r[15] != 0.0f || i + 1 == n_edges) {  // wave-uniform: the contour ends here
        const float dc = fsqrt(bd2);
        rank.insert(r[15], (bs >= 0.0f ? dc : -dc) * orient, 0u);
        bd2 = 3.0e38f; bo = -1.0f; bs = 0.0f;
      }
    }
    uint32_t none;
    const float d = rank.select(none);
    // a point within one quantisation step of the outline convicts nobody
    const bool artefact = cand && (inside ? d < -step : d > step);
    mark = mark | (artefact & (depth >= msdf_depth(other)));
    todo &= todo - 1u;
  }
  if (live) out[(size_t)y * w + x] = mark ? ((c & 0xFF000000u) | (uint32_t)msdf_median(c) * 0x010101u) : c;
}

// ------------------------------------------------------------------ fdh_put_glyph_outlines: a batch of fields in one launch
// (the specification: include_glyphs/figdraw_hip_glyphs.h).  The four bodies above, each on one glyph's slice of a concatenated field buffer.  The grid
// is 1-D over all 8 x 8 tiles of all glyphs; the host wrote which glyph a tile belongs to (tile_glyph) and the glyph's record (msdf::BatchGlyph,
// fdh_msdf_host.h).  Both depend on blockIdx alone: scalar loads, as the edge records behind them.  A tile lies inside its glyph's
// tile grid, so a store goes to the glyph's own w x h texels and nowhere else.
#define FDH_MSDF_BATCH_TILE                                                                      \
  const msdf::BatchGlyph g = glyphs[tile_glyph[blockIdx.x]];                                     \
  const int tile = (int)(blockIdx.x - g.first_tile), tiles_x = (g.w + 7) / 8;                    \
  const int ty0 = tile / tiles_x * 8, tx0 = (tile - tile / tiles_x * tiles_x) * 8;               \
  const float* __restrict__ rec = edges + (size_t)g.edge_off * msdf::kEdgeFloats
__global__ __launch_bounds__(64) void k_msdf_generate_batch(const float* __restrict__ edges, const msdf::BatchGlyph* __restrict__ glyphs,
                                                            const uint32_t* __restrict__ tile_glyph, uint32_t* __restrict__ out) {
  FDH_MSDF_BATCH_TILE;
  msdf_generate_tile(rec, g.n_edges, g.w, g.h, g.orient, g.inv_range, out + g.field_off, tx0, ty0);
}
__global__ __launch_bounds__(64) void k_msdf_generate_union_batch(const float* __restrict__ edges, const msdf::BatchGlyph* __restrict__ glyphs,
                                                                  const uint32_t* __restrict__ tile_glyph, uint32_t* __restrict__ out) {
  FDH_MSDF_BATCH_TILE;
  msdf_generate_union_tile(rec, g.n_edges, g.w, g.h, g.orient, g.inv_range, out + g.field_off, tx0, ty0);
}
__global__ __launch_bounds__(64) void k_msdf_correct_batch(const float* __restrict__ edges, const msdf::BatchGlyph* __restrict__ glyphs,
                                                           const uint32_t* __restrict__ tile_glyph, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  FDH_MSDF_BATCH_TILE;
  msdf_correct_tile(rec, g.n_edges, g.w, g.h, g.orient, g.step, in + g.field_off, out + g.field_off, tx0, ty0);
}
__global__ __launch_bounds__(64) void k_msdf_correct_union_batch(const float* __restrict__ edges, const msdf::BatchGlyph* __restrict__ glyphs,
                                                                 const uint32_t* __restrict__ tile_glyph, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  FDH_MSDF_BATCH_TILE;
  msdf_correct_union_tile(rec, g.n_edges, g.w, g.h, g.orient, g.step, in + g.field_off, out + g.field_off, tx0, ty0);
}
#undef FDH_MSDF_BATCH_TILE

void launch_msdf_generate_batch(hipStream_t s, bool overlap, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, uint32_t* out) {
  if (n_tiles <= 0) return;
  if (overlap) FDH_LAUNCH(k_msdf_generate_union_batch, dim3(n_tiles), dim3(64), 0, s, edges, glyphs, tile_glyph, out);
  else FDH_LAUNCH(k_msdf_generate_batch, dim3(n_tiles), dim3(64), 0, s, edges, glyphs, tile_glyph, out);
}
void launch_msdf_correct_batch(hipStream_t s, bool overlap, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* in,
                               uint32_t* out) {
  if (n_tiles <= 0) return;
  if (overlap) FDH_LAUNCH(k_msdf_correct_union_batch, dim3(n_tiles), dim3(64), 0, s, edges, glyphs, tile_glyph, in, out);
  else FDH_LAUNCH(k_msdf_correct_batch, dim3(n_tiles), dim3(64), 0, s, edges, glyphs, tile_glyph, in, out);
}

}  // namespace fdh
