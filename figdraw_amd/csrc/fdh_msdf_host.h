// fdh_msdf_host.h -- the host half of distance-field generation (fdh_put_glyph_outline with FDH_GLYPH_MTSDF; the specification is the
// comment at that flag in include/figdraw_hip.h, steps 1 to 3, and of step 6 which contours are filled): an outline becomes contours, an
// orientation, coloured edges, and the record k_msdf_generate reads per edge.  Plain C++, no HIP: tests/msdf_emu compiles it as it
// stands.  All decisions (corners, the orientation, the split points) are taken in double on the float32 coordinates the caller
// passed, so that a second implementation in double reproduces them exactly.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace fdh {
namespace msdf {

// The edge record, kEdgeFloats floats:
//   0..5   P0, P1, P2 (a line: P1 = P0)
//   6      the colour mask as a number (R = 1, G = 2, B = 4)      7  kind: 0 line, 1 quadratic
//   8..9   a = P1 - P0 (a line: e = P2 - P0)                      10..11  b = P0 - 2 P1 + P2 (a line: 0)
//   12     1 / |b|^2 (a line: 1 / |e|^2)     13  kx = (a . b) / |b|^2     14  2 |a|^2
//   15     0 inside a contour; on a contour's last edge +1 when the contour is filled, -1 when it is a hole (step 6 of the
//          specification: FDH_GLYPH_MTSDF_OVERLAP; k_msdf_generate and k_msdf_correct do not read it)
//   16..19 the unit tangents at t = 0 and at t = 1
//   20..23 the box of the control points: x0, y0, x1, y1
// 8..14 are what the cubic of the nearest point owes to the curve alone (sd_bezierN in fdh_device.h computes the same per draw), in
// float32 and in that function's order of operations.
constexpr int kEdgeFloats = 24;
constexpr int kMaxSegments = 65535;
enum Colour { kRed = 1, kGreen = 2, kBlue = 4, kYellow = 3, kMagenta = 5, kCyan = 6, kWhite = 7 };

struct Edge {
  float p[6];  // P0, P1, P2 (a line: P1 = P0)
  bool line;
  int colour;
};

inline void unit(double x, double y, double* ox, double* oy) {
  const double l = std::sqrt(x * x + y * y);
  *ox = l > 0.0 ? x / l : 0.0;
  *oy = l > 0.0 ? y / l : 0.0;
}
// the tangent directions at the ends (not normalised): a control point on an end leaves the chord
inline void end_tangents(const Edge& e, double t0[2], double t1[2]) {
  const double cx = (double)e.p[4] - e.p[0], cy = (double)e.p[5] - e.p[1];
  t0[0] = t1[0] = cx; t0[1] = t1[1] = cy;
  if (e.line) return;
  const double ax = (double)e.p[2] - e.p[0], ay = (double)e.p[3] - e.p[1], bx = (double)e.p[4] - e.p[2], by = (double)e.p[5] - e.p[3];
  if (ax != 0.0 || ay != 0.0) { t0[0] = ax; t0[1] = ay; }
  if (bx != 0.0 || by != 0.0) { t1[0] = bx; t1[1] = by; }
}
inline double lerp(double a, double b, double t) { return a + (b - a) * t; }
// the point at t by de Casteljau, rounded to float32
inline void point_at(const Edge& e, double t, float out[2]) {
  for (int k = 0; k < 2; k++) {
    if (e.line) out[k] = (float)lerp(e.p[k], e.p[4 + k], t);
    else out[k] = (float)lerp(lerp(e.p[k], e.p[2 + k], t), lerp(e.p[2 + k], e.p[4 + k], t), t);
  }
}
// part k of 3 (t in [k / 3, (k + 1) / 3]): end points on the curve, the control point the blossom b(t0, t1); the outer ends stay bit-exact
inline Edge third(const Edge& e, int k) {
  const double t0 = k / 3.0, t1 = (k + 1) / 3.0;
  Edge o = e;
  if (k > 0) point_at(e, t0, &o.p[0]);
  if (k < 2) point_at(e, t1, &o.p[4]);
  for (int c = 0; c < 2; c++) {
    if (e.line) o.p[2 + c] = o.p[c];
    else o.p[2 + c] = (float)lerp(lerp(e.p[c], e.p[2 + c], t0), lerp(e.p[2 + c], e.p[4 + c], t0), t1);
  }
  return o;
}

// step 3 for one closed contour (edges in order); may replace it by its split form.  Written once for both edge types (this file's and
// fdh_msdf_cubic_host.h's): end_tangents and third are the overloads of the edge's own namespace.
template <typename E>
inline void colour_contour(std::vector<E>& c) {
  const int m = (int)c.size();
  std::vector<int> corners;
  const double kSin3 = std::sin(3.0);
  for (int i = 0; i < m; i++) {  // vertex i: where edge i - 1 ends and edge i starts
    double a0[2], a1[2], b0[2], b1[2], ix, iy, ox, oy;
    end_tangents(c[(i + m - 1) % m], a0, a1);
    end_tangents(c[i], b0, b1);
    unit(a1[0], a1[1], &ix, &iy);
    unit(b0[0], b0[1], &ox, &oy);
    const double dot = ix * ox + iy * oy, cross = ix * oy - iy * ox;
    if (dot <= 0.0 || std::fabs(cross) > kSin3) corners.push_back(i);
  }
  static const int cycle[3] = {kMagenta, kYellow, kCyan};
  const int n = (int)corners.size();
  if (n == 0) {
    for (E& e : c) e.colour = kWhite;
  } else if (n == 1) {
    std::vector<E> r;  // from the corner round
    for (int j = 0; j < m; j++) {
      const E& e = c[(corners[0] + j) % m];
      if (m >= 3) r.push_back(e);
      else for (int k = 0; k < 3; k++) r.push_back(third(e, k));
    }
    const int mm = (int)r.size();
    for (int j = 0; j < mm; j++) r[j].colour = cycle[3 * j / mm];
    c.swap(r);
  } else {
    int run = -1, next = 0;  // walk from the first corner; `next`: index into corners of the corner ahead
    for (int j = 0; j < m; j++) {
      const int i = (corners[0] + j) % m;
      if (next < n && corners[next] == i) { run++; next++; }
      c[i].colour = (run == n - 1 && n % 3 == 1) ? (int)kYellow : cycle[run % 3];
    }
  }
}

struct Shape {
  std::vector<Edge> edges;   // every contour's edges, contour after contour
  std::vector<int> contour;  // the contour of each edge
  std::vector<bool> filled;  // per contour, step 6: orient * (its own area) >= 0; otherwise the contour is a hole
  double orient = 1.0;       // the sign of the total area
};

// steps 1 to 3.  false: an open contour
inline bool build_shape(const float* segs, int n, Shape* out) {
  out->edges.clear(); out->contour.clear(); out->filled.clear(); out->orient = 1.0;
  std::vector<Edge> cur;
  std::vector<double> areas;  // per contour: step 2's sum over its own edges
  int n_contours = 0;
  double area = 0.0, own = 0.0;
  for (int i = 0; i < n; i++) {
    const float* q = segs + 6 * (size_t)i;
    Edge e{};
    e.line = q[2] != q[2];
    e.p[0] = q[0]; e.p[1] = q[1]; e.p[4] = q[4]; e.p[5] = q[5];
    e.p[2] = e.line ? q[0] : q[2]; e.p[3] = e.line ? q[1] : q[3];
    if (!e.line) {  // a quadratic without curvature is the line between its ends; so is one whose control point lies on their line, on an end or beyond it
      const double bx = (double)q[0] - 2.0 * (double)q[2] + (double)q[4], by = (double)q[1] - 2.0 * (double)q[3] + (double)q[5];
      const double ax = (double)q[2] - q[0], ay = (double)q[3] - q[1], cx = (double)q[4] - q[0], cy = (double)q[5] - q[1];
      const double ex = (double)q[4] - q[2], ey = (double)q[5] - q[3];
      const bool folded = ax * cy == ay * cx && !(ax * ex > 0.0 || ay * ey > 0.0);  // (products compared one by one: nothing to contract)
      if (bx * bx + by * by <= 1e-6 || folded) { e.line = true; e.p[2] = e.p[0]; e.p[3] = e.p[1]; }
    }
    if (e.line && e.p[0] == e.p[4] && e.p[1] == e.p[5]) continue;  // zero length
    if (!cur.empty() && (cur.back().p[4] != e.p[0] || cur.back().p[5] != e.p[1])) return false;
    cur.push_back(e);
    const double x0 = e.p[0], y0 = e.p[1], x1 = e.p[4], y1 = e.p[5];
    const double chord = 0.5 * (x0 * y1 - x1 * y0), bow = e.line ? 0.0 : (((double)e.p[2] - x0) * (y1 - y0) - ((double)e.p[3] - y0) * (x1 - x0)) / 3.0;
    area += chord; own += chord;
    if (!e.line) { area += bow; own += bow; }
    if (e.p[4] == cur.front().p[0] && e.p[5] == cur.front().p[1]) {
      colour_contour(cur);
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

// the kernel's records
inline void edge_records(const Shape& s, std::vector<float>* rec) {
  rec->assign(s.edges.size() * (size_t)kEdgeFloats, 0.0f);
  for (size_t i = 0; i < s.edges.size(); i++) {
    const Edge& e = s.edges[i];
    float* r = rec->data() + i * kEdgeFloats;
    for (int k = 0; k < 6; k++) r[k] = e.p[k];
    r[6] = (float)e.colour;
    r[7] = e.line ? 0.0f : 1.0f;
    if (e.line) {
      const float ex = e.p[4] - e.p[0], ey = e.p[5] - e.p[1];
      r[8] = ex; r[9] = ey;
      r[12] = 1.0f / (ex * ex + ey * ey);
    } else {
      const float ax = e.p[2] - e.p[0], ay = e.p[3] - e.p[1];
      const float bx = e.p[0] - 2.0f * e.p[2] + e.p[4], by = e.p[1] - 2.0f * e.p[3] + e.p[5];
      const float kk = 1.0f / (bx * bx + by * by);
      r[8] = ax; r[9] = ay; r[10] = bx; r[11] = by;
      r[12] = kk;
      r[13] = kk * (ax * bx + ay * by);
      r[14] = 2.0f * (ax * ax + ay * ay);
    }
    double t0[2], t1[2], ux, uy;
    end_tangents(e, t0, t1);
    unit(t0[0], t0[1], &ux, &uy); r[16] = (float)ux; r[17] = (float)uy;
    unit(t1[0], t1[1], &ux, &uy); r[18] = (float)ux; r[19] = (float)uy;
    if (i + 1 == s.edges.size() || s.contour[i + 1] != s.contour[i]) r[15] = s.filled[(size_t)s.contour[i]] ? 1.0f : -1.0f;
    r[20] = std::fmin(e.p[0], std::fmin(e.p[2], e.p[4])); r[21] = std::fmin(e.p[1], std::fmin(e.p[3], e.p[5]));
    r[22] = std::fmax(e.p[0], std::fmax(e.p[2], e.p[4])); r[23] = std::fmax(e.p[1], std::fmax(e.p[3], e.p[5]));
  }
}

// fdh_put_glyph_outlines (include_glyphs/figdraw_hip_glyphs.h): one glyph of a batch as the batched kernels read it, 16 words.  The glyphs' edge
// records lie one after the other in one buffer, their w x h fields one after the other in another (and in its twin: the correction and the
// level chain go from one to the other inside the glyph's own region); the 8 x 8 tiles of all glyphs are numbered through, row-major
// inside a glyph, and a table of one word per tile names the tile's glyph.
struct BatchGlyph {
  uint32_t edge_off;   // the glyph's first record, in records
  int32_t n_edges;
  int32_t w, h;
  float orient;        // the sign of the outline's area
  float inv_range;     // 1 / range and range / 255 as the single launchers pass them
  float step;
  uint32_t field_off;  // the glyph's first texel in the field buffers
  uint32_t first_tile;
  int32_t x, y;        // where the field goes in level 0 of the atlas
  uint32_t owner_off;  // the glyph's first bit in the table of owned texels (k_atlas_blit_batch), per level from kOwnerLevel on
  uint32_t pad[4];
};
static_assert(sizeof(BatchGlyph) == 64, "BatchGlyph is 16 words");
// Up to this level two glyphs' rectangles cannot meet: the packer keeps 8 texels between them, and level l places ceil(w / 2^l) texels at
// x >> l, which ends at most at ceil((x + w) / 2^l) <= (x + w + 8) >> l while 2^l - 1 <= 8.  From this level on they can, and the later put wins.
constexpr int kOwnerLevel = 4;

}  // namespace msdf
}  // namespace fdh
