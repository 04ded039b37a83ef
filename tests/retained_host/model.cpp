// model.cpp -- class RetainedScene (figdraw_amd/csrc/fdh_retained.cpp) against a naive mirror, as a stand-alone program: no context, no
// device, no HIP header.  tests/test_retained_host.py compiles it with fdh_retained.cpp under AddressSanitizer + UBSan and runs it.
//
// The mirror keeps, for every node, PRIVATE copies of what the node's ranges into the side arrays stand for: its glyphs, their variant
// ids, its drawable ops with their control points, its text rectangles.  A seeded script of edits goes to both; after every step
//   1. every node's ranges in view() resolve to the mirror's content,
//   2. roots and parents equal the mirror's,
//   3. the dirty flags are exactly those of the roots whose before-or-after root set the edit touched (and of new roots),
//   4. every cached PickTag::id of a clean root still names the same node (replace_root compacts the node array),
//   5. a side array holds at most 4096 entries or less than twice what the nodes still reference,
//   6. the settings latch reports a change exactly when the glyph-variant table has just appeared,
// and an edit that fails leaves the state byte-equal to a snapshot taken before it.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "fdh_retained.h"

using namespace fdh;

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d (%s) step %d: ", __FILE__, __LINE__, #c, g_step); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)
static int g_step = -1;

// ------------------------------------------------------------------ the mirror
struct MOp { FdhDrawOp op; std::vector<float> ctrl; };
struct MNode {
  int64_t uid = 0;
  int parent = -1;  // index into the layer (in a subtree on its way in: into the subtree)
  float box[4] = {0, 0, 0, 0};
  std::vector<FdhGlyph> glyphs;
  std::vector<std::array<int64_t, FDH_GLYPH_VARIANT_STEPS>> var;  // what the glyphs' variant ids must read once a table exists
  std::vector<MOp> ops;
  std::vector<FdhTextRect> rects;
};
struct MRoot { int node = 0; bool dirty = true; std::vector<int64_t> tag_uids; };
struct MLayer { int32_t zlevel = 0; std::vector<MNode> nodes; std::vector<MRoot> roots; };

// the root a node hangs under, by its definition: up the parent chain until a node has none (the mirror never holds a parent that
// is not an earlier node: the edits refuse those)
static std::vector<int> roots_of(const MLayer& L) {
  std::vector<int> ro(L.nodes.size());
  for (size_t i = 0; i < L.nodes.size(); i++) {
    int r = (int)i;
    while (L.nodes[(size_t)r].parent >= 0) r = L.nodes[(size_t)r].parent;
    ro[i] = r;
  }
  return ro;
}

static void mirror_update(MLayer& L, int first, const std::vector<MNode>& fresh) {
  const std::vector<int> before = roots_of(L);
  for (size_t k = 0; k < fresh.size(); k++) { const int64_t uid = L.nodes[(size_t)first + k].uid; L.nodes[(size_t)first + k] = fresh[k]; L.nodes[(size_t)first + k].uid = uid; }
  const std::vector<int> after = roots_of(L);
  for (MRoot& r : L.roots)
    for (size_t i = (size_t)first; i < (size_t)first + fresh.size(); i++)
      if (before[i] == r.node || after[i] == r.node) { r.dirty = true; break; }
}

static void mirror_replace(MLayer& L, int slot, const std::vector<MNode>& sub, bool insert) {
  if (!insert) {
    const std::vector<int> ro = roots_of(L);
    const int old_root = L.roots[(size_t)slot].node;
    std::vector<int> remap(L.nodes.size(), -1);
    std::vector<MNode> kept;
    for (size_t i = 0; i < L.nodes.size(); i++)
      if (ro[i] != old_root) { remap[i] = (int)kept.size(); kept.push_back(L.nodes[i]); }
    for (MNode& n : kept) if (n.parent >= 0) n.parent = remap[(size_t)n.parent];
    std::vector<MRoot> roots;
    int new_slot = -1;
    for (size_t s = 0; s < L.roots.size(); s++) {
      if ((int)s == slot) { new_slot = (int)roots.size(); roots.push_back(MRoot{}); continue; }
      if (remap[(size_t)L.roots[s].node] < 0) continue;  // a listed root that hung inside the removed subtree goes with it
      MRoot r = L.roots[s];
      r.node = remap[(size_t)r.node];
      roots.push_back(r);
    }
    L.nodes.swap(kept);
    L.roots.swap(roots);
    slot = new_slot;
    if (sub.empty()) { L.roots.erase(L.roots.begin() + slot); return; }
  } else {
    if (sub.empty()) return;
    L.roots.insert(L.roots.begin() + slot, MRoot{});
  }
  const int base = (int)L.nodes.size();
  for (size_t i = 0; i < sub.size(); i++) {
    MNode n = sub[i];
    n.parent = i == 0 ? -1 : n.parent + base;
    L.nodes.push_back(n);
  }
  L.roots[(size_t)slot] = MRoot{};
  L.roots[(size_t)slot].node = base;
}

// ------------------------------------------------------------------ an edit's nodes as the C ABI hands them over
struct Marshalled {
  std::vector<FdhFig> figs;
  std::vector<FdhGlyph> glyphs;
  std::vector<int64_t> var;
  std::vector<FdhDrawOp> ops;
  std::vector<float> controls;
  std::vector<FdhTextRect> rects;
  FdhScene side;
};
template <typename T> static T zeroed() { T v; std::memset(&v, 0, sizeof v); return v; }

// (`junk` entries in front of every side array: the ranges do not start at 0; with_table: the side arrays bring variant ids)
static void marshal(const std::vector<MNode>& nodes, bool with_table, int junk, Marshalled& m) {
  m = Marshalled{};
  for (int j = 0; j < junk; j++) {
    m.glyphs.push_back(zeroed<FdhGlyph>()); m.glyphs.back().image_id = -77;
    for (int st = 0; st < FDH_GLYPH_VARIANT_STEPS; st++) m.var.push_back(-78);
    m.ops.push_back(zeroed<FdhDrawOp>()); m.controls.push_back(-1.0f); m.controls.push_back(-2.0f);
    m.rects.push_back(zeroed<FdhTextRect>());
  }
  for (const MNode& n : nodes) {
    FdhFig f = zeroed<FdhFig>();
    f.kind = !n.glyphs.empty() ? FDH_NK_TEXT : (!n.ops.empty() ? FDH_NK_DRAWABLE : FDH_NK_RECTANGLE);
    f.parent = n.parent;
    f.image_id = n.uid;
    for (int k = 0; k < 4; k++) f.box[k] = n.box[k];
    f.glyph_first = (int32_t)m.glyphs.size(); f.glyph_count = (int32_t)n.glyphs.size();
    for (size_t g = 0; g < n.glyphs.size(); g++) {
      m.glyphs.push_back(n.glyphs[g]);
      for (int st = 0; st < FDH_GLYPH_VARIANT_STEPS; st++) m.var.push_back(n.var[g][(size_t)st]);
    }
    f.op_first = (int32_t)m.ops.size(); f.op_count = (int32_t)n.ops.size();
    for (const MOp& o : n.ops) {
      FdhDrawOp op = o.op;
      op.ctrl_first = (int32_t)(m.controls.size() / 2); op.ctrl_count = (int32_t)(o.ctrl.size() / 2);
      m.controls.insert(m.controls.end(), o.ctrl.begin(), o.ctrl.end());
      m.ops.push_back(op);
    }
    f.text_rect_first = (int32_t)m.rects.size(); f.text_rect_count = (int32_t)n.rects.size();
    m.rects.insert(m.rects.end(), n.rects.begin(), n.rects.end());
    m.figs.push_back(f);
  }
  m.side = zeroed<FdhScene>();
  m.side.glyphs = m.glyphs.data(); m.side.n_glyphs = (int32_t)m.glyphs.size();
  m.side.glyph_variant_ids = with_table ? m.var.data() : nullptr;
  m.side.ops = m.ops.data(); m.side.n_ops = (int32_t)m.ops.size();
  m.side.controls = m.controls.data(); m.side.n_controls = (int32_t)(m.controls.size() / 2);
  m.side.text_rects = m.rects.data(); m.side.n_text_rects = (int32_t)m.rects.size();
}

// ------------------------------------------------------------------ random content
static std::mt19937 g_rng(20240607u);
static int rnd(int n) { return (int)(g_rng() % (uint32_t)n); }
static int64_t g_uid = 1000;

// (without a table in the side arrays a glyph's variant ids fall back to its own image)
static MNode random_node(bool with_table, int glyphs = -1) {
  MNode n;
  n.uid = g_uid++;
  for (int k = 0; k < 4; k++) n.box[k] = (float)rnd(500);
  const int kind = glyphs >= 0 ? 0 : rnd(4);
  if (kind == 0) {
    const int ng = glyphs >= 0 ? glyphs : 1 + rnd(6);
    for (int g = 0; g < ng; g++) {
      FdhGlyph gl = zeroed<FdhGlyph>();
      gl.image_id = 1 + rnd(1000); gl.x = (float)rnd(300); gl.y = (float)rnd(40); gl.subpixel_shift = -1.0f;
      n.glyphs.push_back(gl);
      std::array<int64_t, FDH_GLYPH_VARIANT_STEPS> v;
      for (int st = 0; st < FDH_GLYPH_VARIANT_STEPS; st++) v[(size_t)st] = with_table ? 100000 + rnd(100000) : gl.image_id;
      n.var.push_back(v);
    }
    for (int r = rnd(3); r > 0; r--) { FdhTextRect t = zeroed<FdhTextRect>(); t.x = (float)rnd(90); t.w = 1.0f + (float)rnd(50); t.h = 2.0f; t.kind = rnd(2); n.rects.push_back(t); }
  } else if (kind == 1) {
    for (int o = 1 + rnd(3); o > 0; o--) {
      MOp op; op.op = zeroed<FdhDrawOp>();
      op.op.kind = rnd(2) ? FDH_DK_BEZIER : FDH_DK_LINE; op.op.v[0] = (float)rnd(1000);
      if (op.op.kind == FDH_DK_BEZIER) for (int c = 2 * (2 + rnd(3)); c > 0; c--) op.ctrl.push_back((float)rnd(4000));
      n.ops.push_back(op);
    }
  }
  return n;
}
static std::vector<MNode> random_subtree(bool with_table) {
  std::vector<MNode> sub{random_node(with_table)};
  for (int k = rnd(4); k > 0; k--) { MNode n = random_node(with_table); n.parent = rnd((int)sub.size()); sub.push_back(n); }
  return sub;
}

// ------------------------------------------------------------------ what is observable of a RetainedScene
constexpr float kUi = 1.0f, kAa = 1.2f;
template <typename T> static void put(std::string& s, const T* p, size_t n) { if (n) s.append(reinterpret_cast<const char*>(p), n * sizeof(T)); s.push_back('|'); }
template <typename T> static void put1(std::string& s, T v) { put(s, &v, 1); }

// every byte the public surface shows, and -- on a copy -- whether the settings latch would report a change
static std::string snapshot(RetainedScene& R) {
  std::string s;
  put1(s, R.valid());
  if (!R.valid()) return s;
  put1(s, R.fw()); put1(s, R.fh()); put1(s, R.clear()); put(s, R.rgba(), 4);
  int64_t walked, reused;
  R.stats(&walked, &reused); put1(s, walked); put1(s, reused);
  const RetainedScene::View V = R.view();
  const FdhScene& v = V.scene;
  put(s, v.glyphs, (size_t)v.n_glyphs); put1(s, v.glyph_variant_ids != nullptr);
  if (v.glyph_variant_ids) put(s, v.glyph_variant_ids, (size_t)v.n_glyphs * FDH_GLYPH_VARIANT_STEPS);
  put(s, v.ops, (size_t)v.n_ops); put(s, v.controls, 2 * (size_t)v.n_controls); put(s, v.text_rects, (size_t)v.n_text_rects);
  for (size_t l = 0; l < R.n_layers(); l++) {
    const RetainedLayer& D = R.layer(l);
    put1(s, D.zlevel); put(s, D.nodes.data(), D.nodes.size()); put(s, D.roots.data(), D.roots.size());
    for (const RetainedRoot& C : D.cache) {
      put1(s, C.dirty); put1(s, C.cacheable); put1(s, C.tagged); put(s, C.tags.data(), C.tags.size()); put(s, C.recs.data(), C.recs.size());
      put1(s, C.fragments); put1(s, C.atlas_epoch);
    }
  }
  RetainedScene copy = R;
  put1(s, copy.latch_settings(kUi, kAa, false, false));
  return s;
}

struct SideUse { size_t glyphs = 0, ops = 0, rects = 0; };
static SideUse live_entries(const MLayer* M, size_t n_layers) {
  SideUse u;
  for (size_t l = 0; l < n_layers; l++)
    for (const MNode& n : M[l].nodes) { u.glyphs += n.glyphs.size(); u.ops += n.ops.size(); u.rects += n.rects.size(); }
  return u;
}

// checks 1 - 5 of the header
static void check_against(RetainedScene& R, const MLayer* M, size_t n_layers) {
  const RetainedScene::View V = R.view();
  const FdhScene& v = V.scene;
  CHECK((size_t)v.n_layers == n_layers && R.n_layers() == n_layers, "layers");
  const bool table = v.glyph_variant_ids != nullptr;
  for (size_t l = 0; l < n_layers; l++) {
    const FdhLayer& L = v.layers[l];
    const MLayer& W = M[l];
    CHECK(L.zlevel == W.zlevel && (size_t)L.n_nodes == W.nodes.size() && (size_t)L.n_roots == W.roots.size(), "layer %zu: %d nodes, %d roots; the mirror has %zu, %zu", l, L.n_nodes, L.n_roots, W.nodes.size(), W.roots.size());
    for (size_t i = 0; i < W.nodes.size(); i++) {
      const FdhFig& f = L.nodes[i];
      const MNode& n = W.nodes[i];
      CHECK(f.image_id == n.uid && f.parent == n.parent && std::memcmp(f.box, n.box, sizeof f.box) == 0, "layer %zu node %zu: uid %lld parent %d, the mirror has %lld, %d", l, i, (long long)f.image_id, f.parent, (long long)n.uid, n.parent);
      CHECK((size_t)f.glyph_count == n.glyphs.size() && (n.glyphs.empty() || (f.glyph_first >= 0 && f.glyph_first + f.glyph_count <= v.n_glyphs)), "node %zu: glyph range", i);
      for (size_t g = 0; g < n.glyphs.size(); g++) {
        const FdhGlyph& a = v.glyphs[(size_t)f.glyph_first + g];
        CHECK(a.image_id == n.glyphs[g].image_id && a.x == n.glyphs[g].x && a.y == n.glyphs[g].y && a.subpixel_shift == n.glyphs[g].subpixel_shift, "node %zu glyph %zu", i, g);
        for (int st = 0; table && st < FDH_GLYPH_VARIANT_STEPS; st++)
          CHECK(v.glyph_variant_ids[((size_t)f.glyph_first + g) * FDH_GLYPH_VARIANT_STEPS + (size_t)st] == n.var[g][(size_t)st], "node %zu glyph %zu variant %d", i, g, st);
        CHECK(table || n.var[g][0] == n.glyphs[g].image_id, "node %zu glyph %zu came with variant ids, and the scene has no table", i, g);
      }
      CHECK((size_t)f.op_count == n.ops.size() && (n.ops.empty() || (f.op_first >= 0 && f.op_first + f.op_count <= v.n_ops)), "node %zu: op range", i);
      for (size_t o = 0; o < n.ops.size(); o++) {
        const FdhDrawOp& a = v.ops[(size_t)f.op_first + o];
        const MOp& b = n.ops[o];
        CHECK(a.kind == b.op.kind && a.v[0] == b.op.v[0] && (size_t)a.ctrl_count == b.ctrl.size() / 2, "node %zu op %zu", i, o);
        CHECK(b.ctrl.empty() || (a.ctrl_first >= 0 && a.ctrl_first + a.ctrl_count <= v.n_controls), "node %zu op %zu: control range", i, o);
        for (size_t c = 0; c < b.ctrl.size(); c++) CHECK(v.controls[2 * (size_t)a.ctrl_first + c] == b.ctrl[c], "node %zu op %zu control %zu", i, o, c);
      }
      CHECK((size_t)f.text_rect_count == n.rects.size() && (n.rects.empty() || (f.text_rect_first >= 0 && f.text_rect_first + f.text_rect_count <= v.n_text_rects)), "node %zu: text-rect range", i);
      for (size_t t = 0; t < n.rects.size(); t++) {
        const FdhTextRect& a = v.text_rects[(size_t)f.text_rect_first + t];
        CHECK(a.x == n.rects[t].x && a.w == n.rects[t].w && a.h == n.rects[t].h && a.kind == n.rects[t].kind, "node %zu text rect %zu", i, t);
      }
    }
    const RetainedLayer& D = R.layer(l);
    CHECK(D.cache.size() == W.roots.size(), "layer %zu: cache entries", l);
    for (size_t s = 0; s < W.roots.size(); s++) {
      CHECK(L.root_ids[s] == W.roots[s].node, "layer %zu root slot %zu: node %d, the mirror has %d", l, s, L.root_ids[s], W.roots[s].node);
      CHECK(D.cache[s].dirty == W.roots[s].dirty, "layer %zu root slot %zu: dirty %d, the mirror has %d", l, s, (int)D.cache[s].dirty, (int)W.roots[s].dirty);
      if (D.cache[s].dirty) continue;
      CHECK(D.cache[s].tags.size() == W.roots[s].tag_uids.size(), "layer %zu root slot %zu: tags", l, s);
      for (size_t k = 0; k < D.cache[s].tags.size(); k++) {
        const int32_t id = D.cache[s].tags[k].id;
        CHECK(id >= 0 && id < L.n_nodes && L.nodes[id].image_id == W.roots[s].tag_uids[k], "layer %zu root slot %zu tag %zu names node %d", l, s, k, id);
      }
    }
  }
  const SideUse live = live_entries(M, n_layers);
  auto bounded = [](size_t have, size_t live_n) { return have <= 4096 || have < 2 * live_n; };
  CHECK(bounded((size_t)v.n_glyphs, live.glyphs), "%d glyphs for %zu live", v.n_glyphs, live.glyphs);
  CHECK(bounded((size_t)v.n_ops, live.ops), "%d ops for %zu live", v.n_ops, live.ops);
  CHECK(bounded((size_t)v.n_text_rects, live.rects), "%d text rects for %zu live", v.n_text_rects, live.rects);
}

// what fdh_scene_render leaves in the caches, as far as the edits care: every root clean, its records' tags naming its nodes
static void fake_render(RetainedScene& R, MLayer* M, size_t n_layers) {
  for (size_t l = 0; l < n_layers; l++) {
    const std::vector<int> ro = roots_of(M[l]);
    for (size_t s = 0; s < M[l].roots.size(); s++) {
      RetainedRoot& C = R.cache(l, s);
      C.dirty = false; C.cacheable = true; C.tagged = true;
      C.tags.clear(); M[l].roots[s].tag_uids.clear();
      for (size_t i = 0; i < ro.size(); i++)
        if (ro[i] == M[l].roots[s].node) { C.tags.push_back(PickTag{M[l].zlevel, (int32_t)i}); M[l].roots[s].tag_uids.push_back(M[l].nodes[i].uid); }
      M[l].roots[s].dirty = false;
    }
  }
}

static void retain_mirror(RetainedScene& R, const MLayer* M, size_t n_layers, bool with_table, std::vector<Marshalled>& keep) {
  // (one side-array set per layer's nodes would do for the C ABI; retain takes ONE scene: marshal all layers' nodes together)
  std::vector<MNode> all;
  for (size_t l = 0; l < n_layers; l++) all.insert(all.end(), M[l].nodes.begin(), M[l].nodes.end());
  keep.assign(1, Marshalled{});
  marshal(all, with_table, 0, keep[0]);
  std::vector<FdhLayer> layers(n_layers);
  std::vector<std::vector<int32_t>> roots(n_layers);
  size_t at = 0;
  for (size_t l = 0; l < n_layers; l++) {
    for (const MRoot& r : M[l].roots) roots[l].push_back(r.node);
    layers[l] = FdhLayer{M[l].zlevel, (int32_t)M[l].nodes.size(), (int32_t)roots[l].size(), 0, keep[0].figs.data() + at, roots[l].data()};
    at += M[l].nodes.size();
  }
  FdhScene sc = keep[0].side;
  sc.layers = layers.data(); sc.n_layers = (int32_t)n_layers;
  const float rgba[4] = {0.25f, 0.5f, 0.75f, 1.0f};
  R.retain(&sc, 640.0f, 480.0f, true, rgba);
}

template <typename F> static bool throws(F f) {
  try { f(); } catch (const Error&) { return true; }
  return false;
}

int main() {
  constexpr size_t NL = 2;
  MLayer M[NL];
  M[0].zlevel = 0; M[1].zlevel = 5;
  for (size_t l = 0; l < NL; l++)
    for (int r = 0; r < (l == 0 ? 12 : 3); r++) {
      std::vector<MNode> sub = random_subtree(false);
      const int base = (int)M[l].nodes.size();
      for (size_t i = 0; i < sub.size(); i++) { if (i) sub[i].parent += base; M[l].nodes.push_back(sub[i]); }
      MRoot root; root.node = base;
      M[l].roots.push_back(root);
    }
  RetainedScene R;
  std::vector<Marshalled> keep;
  Marshalled m;
  CHECK(throws([&] { R.update_nodes(0, 0, 1, nullptr, nullptr); }) && !R.valid(), "an edit before any retain");
  retain_mirror(R, M, NL, false, keep);
  CHECK(R.latch_settings(kUi, kAa, false, false), "the first render after a retain decomposes everything");
  check_against(R, M, NL);
  fake_render(R, M, NL);

  // ---- the script
  int n_update = 0, n_reparent = 0, n_replace = 0, n_insert = 0, n_remove = 0, n_failed = 0, n_failed_kind[5] = {0, 0, 0, 0, 0}, n_compactions = 0, n_table = 0, n_late_roots = 0;
  const int kSteps = 600, kTableFrom = 250;
  for (g_step = 0; g_step < kSteps; g_step++) {
    const bool with_table = g_step >= kTableFrom;  // from here on the edits' side arrays bring variant ids
    const size_t l = rnd(8) == 0 ? 1 : 0;
    MLayer& W = M[l];
    const bool had_table = R.view().scene.glyph_variant_ids != nullptr;
    const int glyphs_before = R.view().scene.n_glyphs, ops_before = R.view().scene.n_ops;
    const int pick = rnd(100);
    if (pick < 10) {  // an edit that must fail, whole
      const std::string before = snapshot(R);
      std::vector<MNode> sub = random_subtree(with_table);
      sub.insert(sub.begin(), random_node(with_table, 3));  // (glyphs -- after kTableFrom, perhaps the first table -- reach the side arrays before the bad node)
      for (size_t i = 1; i < sub.size(); i++) sub[i].parent = i == 1 ? 0 : sub[i].parent + 1;
      sub.push_back(random_node(with_table, 2)); sub.back().parent = 0;
      marshal(sub, with_table, 2, m);
      int kind = rnd(5);
      if (kind == 2 && W.nodes.size() < sub.size()) kind = 4;
      bool failed = false;
      if (kind == 0) { m.figs.back().glyph_count = 1000; failed = throws([&] { R.replace_root((int)l, rnd((int)W.roots.size()), m.figs.data(), (int)m.figs.size(), &m.side, false); }); }
      else if (kind == 1) { m.figs.back().text_rect_first = -1; m.figs.back().text_rect_count = 1; failed = throws([&] { R.replace_root((int)l, rnd((int)W.roots.size() + 1), m.figs.data(), (int)m.figs.size(), &m.side, true); }); }
      else if (kind == 2) {  // update_nodes: the bad side range at the LAST node of the edit
        const int first = rnd((int)(W.nodes.size() - sub.size() + 1));
        for (size_t i = 0; i < sub.size(); i++) m.figs[i].parent = W.nodes[(size_t)first + i].parent;
        m.figs.back().glyph_first = m.side.n_glyphs - 1;  // (2 glyphs from the last entry on)
        failed = throws([&] { R.update_nodes((int)l, first, (int)m.figs.size(), m.figs.data(), &m.side); });
      } else if (kind == 3) { failed = throws([&] { R.replace_root((int)l, (int)W.roots.size(), m.figs.data(), (int)m.figs.size(), &m.side, false); }); }
      else { m.figs[1].parent = 1; failed = throws([&] { R.replace_root((int)l, 0, m.figs.data(), (int)m.figs.size(), &m.side, true); }); }
      CHECK(failed, "a bad edit (kind %d) went through", kind);
      CHECK(snapshot(R) == before, "a failed edit (kind %d) changed the scene", kind);
      n_failed++; n_failed_kind[kind]++;
    } else if (pick < 45 && !W.nodes.empty()) {  // property updates of a node range (the parents stay)
      const int first = rnd((int)W.nodes.size());
      const int count = std::min(1 + rnd(3), (int)W.nodes.size() - first);
      std::vector<MNode> fresh;
      for (int k = 0; k < count; k++) { fresh.push_back(random_node(with_table)); fresh.back().parent = W.nodes[(size_t)(first + k)].parent; fresh.back().uid = W.nodes[(size_t)(first + k)].uid; }
      marshal(fresh, with_table, rnd(3), m);
      R.update_nodes((int)l, first, count, m.figs.data(), &m.side);
      mirror_update(W, first, fresh);
      n_update++;
    } else if (pick < 55 && W.nodes.size() > 2) {  // a node moves under another parent, perhaps another root's; a listed root may get a parent
      const int i = 1 + rnd((int)W.nodes.size() - 1);
      MNode moved = W.nodes[(size_t)i];
      moved.parent = rnd(4) == 0 ? -1 : rnd(i);
      for (const MRoot& r : W.roots) if (r.node == i && moved.parent >= 0) n_late_roots++;
      marshal({moved}, with_table, 1, m);
      // (the node keeps its content: what marshal() wrote for it is what the mirror holds, but for the variant ids without a table)
      if (!with_table) for (size_t g = 0; g < moved.glyphs.size(); g++) moved.var[g].fill(moved.glyphs[g].image_id);
      R.update_nodes((int)l, i, 1, m.figs.data(), &m.side);
      mirror_update(W, i, {moved});
      n_reparent++;
    } else if (pick < 72 && !W.roots.empty()) {
      const int slot = rnd((int)W.roots.size());
      const std::vector<MNode> sub = random_subtree(with_table);
      marshal(sub, with_table, rnd(3), m);
      R.replace_root((int)l, slot, m.figs.data(), (int)m.figs.size(), &m.side, false);
      mirror_replace(W, slot, sub, false);
      n_replace++;
    } else if (pick < 88 || W.roots.size() < 4) {
      const int slot = rnd((int)W.roots.size() + 1);
      const std::vector<MNode> sub = random_subtree(with_table);
      marshal(sub, with_table, rnd(3), m);
      R.replace_root((int)l, slot, m.figs.data(), (int)m.figs.size(), &m.side, true);
      mirror_replace(W, slot, sub, true);
      n_insert++;
    } else {  // removal: a replacement by nothing
      const int slot = rnd((int)W.roots.size());
      R.replace_root((int)l, slot, nullptr, 0, nullptr, false);
      mirror_replace(W, slot, {}, false);
      n_remove++;
    }
    check_against(R, M, NL);
    const bool has_table = R.view().scene.glyph_variant_ids != nullptr;
    const bool changed = R.latch_settings(kUi, kAa, false, false);
    CHECK(changed == (has_table && !had_table), "the settings latch says %d; the variant table was %d and is %d", (int)changed, (int)had_table, (int)has_table);
    n_table += changed;
    if (R.view().scene.n_glyphs < glyphs_before - 64 || R.view().scene.n_ops < ops_before - 64) n_compactions++;
    if (rnd(3) == 0) fake_render(R, M, NL);
  }

  // ---- animated text: one node's 40 glyphs, its text rectangles and a drawable's ops with their control points, replaced 400 times --
  // 16 000 glyphs appended, far past the 4096-entry threshold; check_against holds the arrays to their bound after every step
  g_step = 10000;
  {
    MLayer& W = M[0];
    std::vector<MNode> sub{random_node(true, 40), random_node(true)};
    sub[1].parent = 0;
    sub[1].glyphs.clear(); sub[1].var.clear(); sub[1].rects.clear(); sub[1].ops.clear();
    for (int o = 0; o < 30; o++) { MOp op; op.op = zeroed<FdhDrawOp>(); op.op.kind = FDH_DK_BEZIER; op.ctrl = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f}; sub[1].ops.push_back(op); }
    marshal(sub, true, 0, m);
    R.replace_root(0, 0, m.figs.data(), (int)m.figs.size(), &m.side, true);
    mirror_replace(W, 0, sub, true);
    fake_render(R, M, NL);
    const int first = W.roots[0].node;
    int shrunk = 0;
    for (int k = 0; k < 400; k++, g_step++) {
      std::vector<MNode> fresh{random_node(true, 40), sub[1]};
      fresh[0].parent = -1; fresh[1].parent = first;
      fresh[0].uid = W.nodes[(size_t)first].uid; fresh[1].uid = W.nodes[(size_t)first + 1].uid;
      for (MOp& op : fresh[1].ops) op.op.v[0] = (float)k;
      for (int r = 0; r < 12; r++) { FdhTextRect t = zeroed<FdhTextRect>(); t.x = (float)k; t.w = 5.0f; t.h = 2.0f; t.kind = 1; fresh[0].rects.push_back(t); }
      marshal(fresh, true, 1, m);
      const int before = R.view().scene.n_glyphs;
      R.update_nodes(0, first, 2, m.figs.data(), &m.side);
      mirror_update(W, first, fresh);
      check_against(R, M, NL);
      if (R.view().scene.n_glyphs < before) shrunk++;  // (an edit only appends: the arrays were rebuilt)
      for (size_t s = 1; s < W.roots.size(); s++) CHECK(!W.roots[s].dirty, "only the animated root is dirty");
    }
    CHECK(shrunk >= 2, "400 x 40 glyphs were appended and the side arrays were rebuilt %d times", shrunk);
    n_compactions += shrunk;
  }

  // ---- the node budget: 32767 nodes per layer (FigIdx is int16)
  g_step = 20000;
  {
    const std::string before = snapshot(R);
    const int room = 32767 - (int)M[1].nodes.size();
    std::vector<MNode> big((size_t)room + 1);
    for (size_t i = 0; i < big.size(); i++) { big[i].uid = g_uid++; big[i].parent = i == 0 ? -1 : 0; }
    marshal(big, false, 0, m);
    CHECK(throws([&] { R.replace_root(1, 0, m.figs.data(), (int)m.figs.size(), &m.side, true); }), "32768 nodes in a layer");
    CHECK(snapshot(R) == before, "the refused insert changed the scene");
    big.pop_back(); m.figs.pop_back();
    R.replace_root(1, 1, m.figs.data(), (int)m.figs.size(), &m.side, true);  // exactly 32767: goes through
    mirror_replace(M[1], 1, big, true);
    check_against(R, M, NL);
    CHECK(M[1].nodes.size() == 32767, "the layer is full");
    const std::string full = snapshot(R);
    marshal({random_node(false)}, false, 0, m);
    CHECK(throws([&] { R.replace_root(1, 0, m.figs.data(), 1, &m.side, true); }) && snapshot(R) == full, "one node more than the budget");
    R.replace_root(1, 1, nullptr, 0, nullptr, false);  // (and out again)
    mirror_replace(M[1], 1, {}, false);
    check_against(R, M, NL);
  }

  // ---- a failing retain after a good one: the old scene stays, byte for byte
  g_step = 30000;
  {
    fake_render(R, M, NL);
    const std::string before = snapshot(R);
    Marshalled one;
    marshal({random_node(false), random_node(false)}, false, 0, one);
    const float rgba[4] = {0, 0, 0, 1};
    FdhScene sc = one.side;
    int32_t root_ids[2] = {0, 2};  // (two nodes: root index 2 is out of range)
    FdhLayer layer{0, 2, 2, 0, one.figs.data(), root_ids};
    sc.layers = &layer; sc.n_layers = 1;
    CHECK(throws([&] { R.retain(&sc, 100.0f, 100.0f, false, rgba); }), "a root index out of range");
    CHECK(snapshot(R) == before, "a failed retain (root index) changed the retained scene");
    root_ids[1] = -1;
    CHECK(throws([&] { R.retain(&sc, 100.0f, 100.0f, false, rgba); }) && snapshot(R) == before, "a failed retain (negative root index)");
    root_ids[1] = 1; one.figs[1].parent = 1;
    CHECK(throws([&] { R.retain(&sc, 100.0f, 100.0f, false, rgba); }) && snapshot(R) == before, "a failed retain (parent)");
    layer.n_nodes = 32768;
    CHECK(throws([&] { R.retain(&sc, 100.0f, 100.0f, false, rgba); }) && snapshot(R) == before, "a failed retain (node budget)");
    check_against(R, M, NL);
    layer.n_nodes = 2; one.figs[1].parent = 0; layer.n_roots = 1;
    R.retain(&sc, 100.0f, 100.0f, false, rgba);  // and a good one replaces it
    CHECK(R.n_layers() == 1 && R.layer(0).nodes.size() == 2 && R.layer(0).cache[0].dirty && R.fw() == 100.0f && !R.clear(), "the new scene");
    CHECK(R.latch_settings(kUi, kAa, false, false), "a fresh scene starts from nothing");
  }

  // ---- variant ids arriving late, on their own: the glyphs retained without a table are back-filled with their own image
  g_step = 40000;
  {
    MLayer T[1];
    T[0].nodes.push_back(random_node(false, 5));
    for (int k = 0; k < 2; k++) { T[0].nodes.push_back(random_node(false, 0)); T[0].nodes.back().parent = 0; }
    T[0].roots.push_back(MRoot{});
    retain_mirror(R, T, 1, false, keep);
    CHECK(R.latch_settings(kUi, kAa, true, true), "first render");
    CHECK(!R.latch_settings(kUi, kAa, true, true) && R.view().scene.glyph_variant_ids == nullptr, "nothing changed, no table");
    {  // an update of all three nodes whose side arrays bring the FIRST table; the bad glyph range is the last node's: nothing stays --
       // not the glyphs and ops of the two nodes before it, not the back-fill, not the table's epoch (the snapshot holds the latch)
      fake_render(R, T, 1);
      const std::string before = snapshot(R);
      std::vector<MNode> fresh{random_node(true, 4), random_node(true), random_node(true, 2)};
      fresh[1].parent = fresh[2].parent = 0;
      fresh[1].ops.resize(1); fresh[1].ops[0].op = zeroed<FdhDrawOp>(); fresh[1].ops[0].op.kind = FDH_DK_BEZIER; fresh[1].ops[0].ctrl = {1.0f, 2.0f, 3.0f, 4.0f};
      marshal(fresh, true, 1, m);
      m.figs[2].glyph_first = m.side.n_glyphs - 1;  // (2 glyphs from the last entry on)
      CHECK(throws([&] { R.update_nodes(0, 0, 3, m.figs.data(), &m.side); }), "a glyph range past the side arrays at the last node of an update");
      CHECK(snapshot(R) == before, "the failed update changed the scene");
      m.figs[2].glyph_first = m.side.n_glyphs - 2; m.figs[2].op_first = m.side.n_ops; m.figs[2].op_count = 1;  // the same with a bad op range
      CHECK(throws([&] { R.update_nodes(0, 0, 3, m.figs.data(), &m.side); }) && snapshot(R) == before, "an op range past the side arrays at the last node of an update");
      check_against(R, T, 1);
      n_failed_kind[2]++;
    }
    const std::vector<MNode> sub{random_node(true, 4)};
    marshal(sub, true, 3, m);
    R.replace_root(0, 1, m.figs.data(), 1, &m.side, true);
    mirror_replace(T[0], 1, sub, true);
    check_against(R, T, 1);  // (the old glyphs' variant ids read image_id, the new ones' what the side arrays brought)
    const RetainedScene::View V = R.view();
    const FdhScene& v = V.scene;
    CHECK(v.glyph_variant_ids && v.glyph_variant_ids[0] == v.glyphs[0].image_id && v.glyph_variant_ids[5 * FDH_GLYPH_VARIANT_STEPS] == sub[0].var[0][0], "the back-fill");
    CHECK(R.latch_settings(kUi, kAa, true, true), "the table's appearance makes every cached record stale");
    CHECK(!R.latch_settings(kUi, kAa, true, true), "... once");
    CHECK(R.latch_settings(kUi, kAa, false, true) && R.latch_settings(2.0f, kAa, false, true) && R.latch_settings(2.0f, 1.0f, false, true) && R.latch_settings(2.0f, 1.0f, false, false) && !R.latch_settings(2.0f, 1.0f, false, false), "each setting is latched");
    n_table++;
  }

  std::printf("steps %d updates %d reparents %d late_roots %d replaces %d inserts %d removes %d failed %d failed_replace_side %d failed_insert_side %d failed_update_last_node %d failed_slot %d failed_parent %d compactions %d tables %d\n",
              kSteps, n_update, n_reparent, n_late_roots, n_replace, n_insert, n_remove, n_failed, n_failed_kind[0], n_failed_kind[1], n_failed_kind[2], n_failed_kind[3], n_failed_kind[4], n_compactions, n_table);
  std::printf("OK\n");
  return 0;
}
