// fdh_msdf_cubic_host.h -- the host half of distance-field generation for outlines that hold cubic segments (fdh_put_glyph_outline_cubic
// with FDH_GLYPH_MTSDF; the specification is the comment in include_glyphs/figdraw_hip_cubic.h, which extends steps 1 to 3 of
// include/figdraw_hip.h): an outline of 8-float segments becomes contours, an orientation, coloured edges, and the record
// k_msdf_generate_cubic reads per edge.  Plain C++, no HIP: tests/msdf_cubic_emu compiles it as it stands.  fdh_msdf_host.h is the same for
// outlines of lines and quadratics; what the two share (unit, lerp, the colours, the segment limit) is taken from there.  All decisions are
// taken in double on the float32 coordinates the caller passed, so that a second implementation in double reproduces them exactly.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "fdh_msdf_host.h"

namespace fdh {
namespace msdf {
namespace cubic {

// The edge record, kCubicEdgeFloats floats.  A line or a quadratic: slots 0..23 are msdf::edge_records' 24 floats, value for value (kind 0
// or 1), the rest 0: the device runs k_msdf.hip's expressions on them.  A cubic, kind 2:
//   0..1   P0          2..3   P1          4..5   P3 (the END point: slots 0, 1, 4, 5 are the ends whatever the kind)          28..29  P2
//   6      the colour mask as a number (R = 1, G = 2, B = 4)      7  kind: 2
//   8..13  B(t) = P0 + c1 t + c2 t^2 + c3 t^3: c1 = 3 (P1 - P0), c2 = 3 (P0 - 2 P1 + P2), c3 = P3 - 3 P2 + 3 P1 - P0
//   24..27 B'(t) = c1 + d1 t + d2 t^2: d1 = 2 c2, d2 = 3 c3          (each taken in double from the float32 points, rounded once)
//   30..33 the same curve from its other end, B(1 - s) = P3 - r1 s + r2 s^2 - c3 s^3: r1 = 3 (P3 - P2), r2 = 3 (P3 - 2 P2 + P1): near t = 1 this
//          form gives B(t) - P3 to its own precision, as the first gives B(t) - P0 near t = 0
//   14     K, the number of intervals the search samples (sample_count below)
//   15     as in fdh_msdf_host.h (no kernel here reads it)
//   16..19 the unit tangents at t = 0 and at t = 1 (step 3's: the first of P1 - P0, P2 - P0, P3 - P0 that is not zero; P3 - P2, P3 - P1, P3 - P0)
//   20..23 the box of the four control points, which bounds the curve: x0, y0, x1, y1
constexpr int kCubicEdgeFloats = 36;
enum Kind { kLine = 0, kQuadratic = 1, kCubic = 2 };

struct Edge {
  float p[8];  // P0, P1, P2, P3; a quadratic: P0, C, C, P3; a line: P0, P0, P0, P3
  int kind;
  int colour;
};

inline Edge make_line(const float a[2], const float b[2]) { return Edge{{a[0], a[1], a[0], a[1], a[0], a[1], b[0], b[1]}, kLine, 0}; }
inline Edge make_quadratic(const float a[2], const float c[2], const float b[2]) { return Edge{{a[0], a[1], c[0], c[1], c[0], c[1], b[0], b[1]}, kQuadratic, 0}; }

// the tangent directions at the ends (not normalised): a control point on an end leaves the next one, then the chord
inline void end_tangents(const Edge& e, double t0[2], double t1[2]) {
  for (int k = 0; k < 2; k++) t0[k] = t1[k] = (double)e.p[6 + k] - e.p[k];
  if (e.kind == kLine) return;
  for (int j = 2; j >= 1; j--) {  // the farther control point first, the nearer one overrides it
    const double ax = (double)e.p[2 * j] - e.p[0], ay = (double)e.p[2 * j + 1] - e.p[1];
    if (ax != 0.0 || ay != 0.0) { t0[0] = ax; t0[1] = ay; }
  }
  for (int j = 1; j <= 2; j++) {
    const double bx = (double)e.p[6] - e.p[2 * j], by = (double)e.p[7] - e.p[2 * j + 1];
    if (bx != 0.0 || by != 0.0) { t1[0] = bx; t1[1] = by; }
  }
}
// the blossom b(r, s, u) of a cubic by de Casteljau (b(t, t, t) is the point at t); a quadratic's is b(r, s)
inline double blossom(const Edge& e, int c, double r, double s, double u) {
  const double p0 = e.p[c], p1 = e.p[2 + c], p2 = e.p[4 + c], p3 = e.p[6 + c];
  if (e.kind == kLine) return lerp(p0, p3, u);
  if (e.kind == kQuadratic) return lerp(lerp(p0, p1, s), lerp(p1, p3, s), u);
  const double q0 = lerp(p0, p1, r), q1 = lerp(p1, p2, r), q2 = lerp(p2, p3, r);
  return lerp(lerp(q0, q1, s), lerp(q1, q2, s), u);
}
// part k of 3 (t in [k / 3, (k + 1) / 3]): end points on the curve, the control points the blossoms b(t0, t0, t1) and b(t0, t1, t1) (a
// quadratic: b(t0, t1)), each rounded to float32; the outer ends stay bit-exact
inline Edge third(const Edge& e, int k) {
  const double t0 = k / 3.0, t1 = (k + 1) / 3.0;
  Edge o = e;
  for (int c = 0; c < 2; c++) {
    if (k > 0) o.p[c] = (float)blossom(e, c, t0, t0, t0);
    if (k < 2) o.p[6 + c] = (float)blossom(e, c, t1, t1, t1);
  }
  for (int c = 0; c < 2; c++) {
    if (e.kind == kLine) o.p[2 + c] = o.p[4 + c] = o.p[c];
    else if (e.kind == kQuadratic) o.p[2 + c] = o.p[4 + c] = (float)blossom(e, c, t0, t0, t1);
    else { o.p[2 + c] = (float)blossom(e, c, t0, t0, t1); o.p[4 + c] = (float)blossom(e, c, t0, t1, t1); }
  }
  return o;
}

struct Shape {
  std::vector<Edge> edges;   // every contour's edges, contour after contour
  std::vector<int> contour;  // the contour of each edge
  std::vector<bool> filled;  // per contour: orient * (its own area) >= 0
  double orient = 1.0;       // the sign of the total area
  bool has_cubic = false;    // a segment of the INPUT is a cubic (c1x and c2x both numbers), whatever step 1 makes of it
};

// does the 8-float outline hold a cubic segment?  (Without one the call is fdh_put_glyph_outline on the same segments.)
inline bool holds_cubic(const float* segs, int n) {
  for (int i = 0; i < n; i++) {
    const float* q = segs + 8 * (size_t)i;
    if (q[2] == q[2] && q[4] == q[4]) return true;
  }
  return false;
}
// a cubic-free outline in the 6-float format of fdh_put_glyph_outline
inline void to_quadratic_format(const float* segs, int n, std::vector<float>* out) {
  out->resize((size_t)n * 6);
  for (int i = 0; i < n; i++) {
    const float* q = segs + 8 * (size_t)i;
    float* o = out->data() + 6 * (size_t)i;
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = q[6]; o[5] = q[7];
  }
}

// step 1's quadratic rules (fdh_msdf_host.h build_shape): a quadratic without curvature, or folded onto the line of its ends, is that line
inline Edge quadratic_or_line(const float p0[2], const float c[2], const float p3[2]) {
  const double bx = (double)p0[0] - 2.0 * (double)c[0] + (double)p3[0], by = (double)p0[1] - 2.0 * (double)c[1] + (double)p3[1];
  const double ax = (double)c[0] - p0[0], ay = (double)c[1] - p0[1], cx = (double)p3[0] - p0[0], cy = (double)p3[1] - p0[1];
  const double ex = (double)p3[0] - c[0], ey = (double)p3[1] - c[1];
  const bool folded = ax * cy == ay * cx && !(ax * ex > 0.0 || ay * ey > 0.0);  // (products compared one by one: nothing to contract)
  if (bx * bx + by * by <= 1e-6 || folded) return make_line(p0, p3);
  return make_quadratic(p0, c, p3);
}

// steps 1 to 3 for n segments of 8 floats.  false: an open contour
inline bool build_shape(const float* segs, int n, Shape* out) {
  out->edges.clear(); out->contour.clear(); out->filled.clear(); out->orient = 1.0; out->has_cubic = false;
  std::vector<Edge> cur;
  std::vector<double> areas;  // per contour: step 2's sum over its own edges
  int n_contours = 0;
  double area = 0.0, own = 0.0;
  for (int i = 0; i < n; i++) {
    const float* q = segs + 8 * (size_t)i;
    const float *p0 = q, *p3 = q + 6;
    Edge e;
    if (q[2] != q[2]) e = make_line(p0, p3);
    else if (q[4] != q[4]) e = quadratic_or_line(p0, q + 2, p3);
    else {
      out->has_cubic = true;
      const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
      const double tx = x3 - 3.0 * x2 + 3.0 * x1 - x0, ty = y3 - 3.0 * y2 + 3.0 * y1 - y0;
      if (x1 == x0 && y1 == y0 && x2 == x0 && y2 == y0 && x3 == x0 && y3 == y0) continue;  // a point
      if (tx * tx + ty * ty <= 1e-6) {  // a quadratic in a cubic's clothes
        const float c[2] = {(float)((3.0 * (x1 + x2) - (x0 + x3)) / 4.0), (float)((3.0 * (y1 + y2) - (y0 + y3)) / 4.0)};
        e = quadratic_or_line(p0, c, p3);
      } else {
        // all four on one line: from P0 both control points lie along the chord; where the chord is a point, along each other
        const double ux = x1 - x0, uy = y1 - y0, vx = x2 - x0, vy = y2 - y0, wx = x3 - x0, wy = y3 - y0;
        const bool closed = wx == 0.0 && wy == 0.0;
        const bool on_line = closed ? ux * vy == uy * vx : (ux * wy == uy * wx && vx * wy == vy * wx);
        if (on_line) e = make_line(p0, p3);
        else e = Edge{{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]}, kCubic, 0};
      }
    }
    if (e.kind == kLine && e.p[0] == e.p[6] && e.p[1] == e.p[7]) continue;  // zero length
    if (!cur.empty() && (cur.back().p[6] != e.p[0] || cur.back().p[7] != e.p[1])) return false;
    cur.push_back(e);
    const double x0 = e.p[0], y0 = e.p[1], x3 = e.p[6], y3 = e.p[7];
    const double chord = 0.5 * (x0 * y3 - x3 * y0);
    double bow = 0.0;
    if (e.kind == kQuadratic) bow = (((double)e.p[2] - x0) * (y3 - y0) - ((double)e.p[3] - y0) * (x3 - x0)) / 3.0;
    if (e.kind == kCubic) {  // the area between the curve and its chord, exactly: (3 u x v + 3 u x w + 6 v x w) / 20, u, v, w = P1, P2, P3 - P0
      const double ux = (double)e.p[2] - x0, uy = (double)e.p[3] - y0, vx = (double)e.p[4] - x0, vy = (double)e.p[5] - y0, wx = x3 - x0, wy = y3 - y0;
      bow = (3.0 * (ux * vy - uy * vx) + 3.0 * (ux * wy - uy * wx) + 6.0 * (vx * wy - vy * wx)) / 20.0;
    }
    area += chord; own += chord;
    if (e.kind != kLine) { area += bow; own += bow; }
    if (e.p[6] == cur.front().p[0] && e.p[7] == cur.front().p[1]) {
      colour_contour(cur);  // (msdf::colour_contour, on these edges)
      for (const Edge& c : cur) { out->edges.push_back(c); out->contour.push_back(n_contours); }
      areas.push_back(own);
      own = 0.0;
      n_contours++;
      cur.clear();
    }
  }
  if (!cur.empty()) return false;
  out->orient = area >= 0.0 ? 1.0 : -1.0;
  for (double a : areas) out->filled.push_back(out->orient * a >= 0.0);
  return true;
}

// K for a cubic: the search evaluates g(t) = (B(t) - p) . B'(t) at K + 1 uniform parameters and refines between them, so an interval must
// not hold two minima of the distance.  That follows how much the curve turns (the turning of the control polygon bounds the curve's) and
// how unevenly t moves along it (|B'| at the ends and in the middle: where the curve all but halts, equal steps of t crowd together).
// 8 for a plain arc, up to 32.
inline int sample_count(const Edge& e) {
  double turn = 0.0, px = 0.0, py = 0.0;
  bool have = false;
  for (int j = 0; j < 3; j++) {
    const double dx = (double)e.p[2 * j + 2] - e.p[2 * j], dy = (double)e.p[2 * j + 3] - e.p[2 * j + 1];
    if (dx == 0.0 && dy == 0.0) continue;
    if (have) turn += std::fabs(std::atan2(px * dy - py * dx, px * dx + py * dy));
    px = dx; py = dy; have = true;
  }
  double lo = 1e300, hi = 0.0;
  for (int j = 0; j <= 4; j++) {  // |B'(t)| / 3 at t = 0, 1/4, .., 1
    const double t = j / 4.0, u = 1.0 - t;
    double d[2];
    for (int c = 0; c < 2; c++)
      d[c] = u * u * ((double)e.p[2 + c] - e.p[c]) + 2.0 * u * t * ((double)e.p[4 + c] - e.p[2 + c]) + t * t * ((double)e.p[6 + c] - e.p[4 + c]);
    const double s = std::sqrt(d[0] * d[0] + d[1] * d[1]);
    lo = std::fmin(lo, s); hi = std::fmax(hi, s);
  }
  const double ratio = lo > 0.0 ? hi / lo : 1e9;
  const int k = 8 + 4 * (int)std::ceil(turn / 0.7853981633974483) + 2 * (int)std::ceil(std::fmin(std::log2(std::fmax(ratio, 1.0)), 6.0));
  return k > 32 ? 32 : k;
}

// the kernels' records
inline void edge_records(const Shape& s, std::vector<float>* rec) {
  rec->assign(s.edges.size() * (size_t)kCubicEdgeFloats, 0.0f);
  for (size_t i = 0; i < s.edges.size(); i++) {
    const Edge& e = s.edges[i];
    float* r = rec->data() + i * kCubicEdgeFloats;
    r[6] = (float)e.colour;
    r[7] = (float)e.kind;
    if (e.kind == kCubic) {
      r[0] = e.p[0]; r[1] = e.p[1]; r[2] = e.p[2]; r[3] = e.p[3]; r[4] = e.p[6]; r[5] = e.p[7]; r[28] = e.p[4]; r[29] = e.p[5];
      for (int c = 0; c < 2; c++) {
        const double p0 = e.p[c], p1 = e.p[2 + c], p2 = e.p[4 + c], p3 = e.p[6 + c];
        const double c1 = 3.0 * (p1 - p0), c2 = 3.0 * (p0 - 2.0 * p1 + p2), c3 = p3 - 3.0 * p2 + 3.0 * p1 - p0;
        r[8 + c] = (float)c1; r[10 + c] = (float)c2; r[12 + c] = (float)c3;
        r[24 + c] = (float)(2.0 * c2); r[26 + c] = (float)(3.0 * c3);
        r[30 + c] = (float)(3.0 * (p3 - p2)); r[32 + c] = (float)(3.0 * (p3 - 2.0 * p2 + p1));
      }
      r[14] = (float)sample_count(e);
    } else {  // msdf::edge_records' expressions, in float32 and in their order
      const float P[6] = {e.p[0], e.p[1], e.p[2], e.p[3], e.p[6], e.p[7]};
      for (int k = 0; k < 6; k++) r[k] = P[k];
      if (e.kind == kLine) {
        const float ex = P[4] - P[0], ey = P[5] - P[1];
        r[8] = ex; r[9] = ey;
        r[12] = 1.0f / (ex * ex + ey * ey);
      } else {
        const float ax = P[2] - P[0], ay = P[3] - P[1];
        const float bx = P[0] - 2.0f * P[2] + P[4], by = P[1] - 2.0f * P[3] + P[5];
        const float kk = 1.0f / (bx * bx + by * by);
        r[8] = ax; r[9] = ay; r[10] = bx; r[11] = by;
        r[12] = kk;
        r[13] = kk * (ax * bx + ay * by);
        r[14] = 2.0f * (ax * ax + ay * ay);
      }
    }
    double t0[2], t1[2], ux, uy;
    end_tangents(e, t0, t1);
    unit(t0[0], t0[1], &ux, &uy); r[16] = (float)ux; r[17] = (float)uy;
    unit(t1[0], t1[1], &ux, &uy); r[18] = (float)ux; r[19] = (float)uy;
    if (i + 1 == s.edges.size() || s.contour[i + 1] != s.contour[i]) r[15] = s.filled[(size_t)s.contour[i]] ? 1.0f : -1.0f;
    r[20] = std::fmin(std::fmin(e.p[0], e.p[2]), std::fmin(e.p[4], e.p[6])); r[21] = std::fmin(std::fmin(e.p[1], e.p[3]), std::fmin(e.p[5], e.p[7]));
    r[22] = std::fmax(std::fmax(e.p[0], e.p[2]), std::fmax(e.p[4], e.p[6])); r[23] = std::fmax(std::fmax(e.p[1], e.p[3]), std::fmax(e.p[5], e.p[7]));
  }
}

// The coverage path: the lines (x0, y0, x1, y1) of an outline's n segments of 8 floats, appended.  Lines and quadratics: fdh_glyphs.cpp's
// flatten_outline, formula for formula.  A cubic: k uniform chords; the error of a chord over an interval h of t is at most
// h^2 / 8 max |B''|, and max |B''| = 6 max(|P0 - 2 P1 + P2|, |P1 - 2 P2 + P3|): k = ceil(sqrt(0.75 dev / 0.025)), at most 256.
inline int cubic_flatten_count(const float* q) {
  const float ax = q[0] - 2.0f * q[2] + q[4], ay = q[1] - 2.0f * q[3] + q[5], bx = q[2] - 2.0f * q[4] + q[6], by = q[3] - 2.0f * q[5] + q[7];
  const float dev = std::sqrt(std::fmax(ax * ax + ay * ay, bx * bx + by * by));
  const int n = (int)std::ceil(std::sqrt(dev * 30.0f));
  return n < 1 ? 1 : (n > 256 ? 256 : n);
}
inline void flatten_outline(const float* segs, int n, std::vector<float>* lines) {
  for (int i = 0; i < n; i++) {
    const float* q = segs + 8 * (size_t)i;
    if (q[2] != q[2]) { lines->insert(lines->end(), {q[0], q[1], q[6], q[7]}); continue; }
    if (q[4] != q[4]) {
      const float ddx = q[0] - 2.0f * q[2] + q[6], ddy = q[1] - 2.0f * q[3] + q[7];
      const float dev = std::sqrt(ddx * ddx + ddy * ddy);
      int k = (int)std::ceil(std::sqrt(dev * 10.0f));
      k = k < 1 ? 1 : (k > 64 ? 64 : k);
      float px = q[0], py = q[1];
      for (int j = 1; j <= k; j++) {
        const float t = (float)j / (float)k, u = 1.0f - t;
        const float x = j == k ? q[6] : (u * u) * q[0] + (2.0f * u * t) * q[2] + (t * t) * q[6];
        const float y = j == k ? q[7] : (u * u) * q[1] + (2.0f * u * t) * q[3] + (t * t) * q[7];
        lines->insert(lines->end(), {px, py, x, y});
        px = x; py = y;
      }
      continue;
    }
    const int k = cubic_flatten_count(q);
    float px = q[0], py = q[1];
    for (int j = 1; j <= k; j++) {
      const float t = (float)j / (float)k, u = 1.0f - t;
      const float b0 = u * u * u, b1 = 3.0f * u * u * t, b2 = 3.0f * u * t * t, b3 = t * t * t;
      const float x = j == k ? q[6] : b0 * q[0] + b1 * q[2] + b2 * q[4] + b3 * q[6];
      const float y = j == k ? q[7] : b0 * q[1] + b1 * q[3] + b2 * q[5] + b3 * q[7];
      lines->insert(lines->end(), {px, py, x, y});
      px = x; py = y;
    }
  }
}

}  // namespace cubic
}  // namespace msdf
}  // namespace fdh
