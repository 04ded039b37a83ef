// fdh_retained.cpp -- the retained scene: the tree fdh_scene_retain copied and the edits that keep it (fdh_retained.h).  Plain C++.
#include "fdh_retained.h"

#include <algorithm>
#include <string>
#include <utility>

namespace fdh {

// ------------------------------------------------------------------ retained scenes (renderfragments.nim:426-544, common/transfer.nim)
// The reference keeps a base `Renders` and lets the application insert / append / replace fragments of it between frames
// (insertChildren, addChildren, insertRoot, updateFragment :523); its renderer still walks the whole tree every frame.  Here
// the tree lives in the context: fdh_scene_retain copies it, fdh_scene_update_nodes / fdh_scene_replace_root / fdh_scene_insert_root
// edit it, and fdh_scene_render re-decomposes only the roots an edit touched -- the draw records of every other root are
// spliced back from the per-root cache (a memcpy), so a frame after a small edit costs the launches, not a tree walk.

void RetainedScene::rebase_side(FdhFig* nodes, int n, const FdhScene* side) {
  // the new nodes index glyph / op / control / text-rect arrays of `side`: append what they use to the retained arrays
  for (int i = 0; i < n; i++) {
    FdhFig& f = nodes[i];
    if (f.glyph_count > 0) {
      if (!side || !side->glyphs || f.glyph_first < 0 || f.glyph_first + f.glyph_count > side->n_glyphs) throw Error(FDH_ERR_INVALID, "scene update: glyph range outside the side arrays");
      const int base = (int)glyphs_.size();
      glyphs_.insert(glyphs_.end(), side->glyphs + f.glyph_first, side->glyphs + f.glyph_first + f.glyph_count);
      if (!variant_ids_.empty() || side->glyph_variant_ids) {
        // glyphs retained before any variant table existed fall back to their own image, as the new-glyph branch below does.
        // (The table's mere presence changes how renderText treats EVERY glyph under variant positioning -- key lookup with
        // shift 0 instead of the fractional shift -- so records cached without it are stale: table_epoch.)
        if (variant_ids_.empty()) table_epoch_++;
        for (size_t g0 = variant_ids_.size() / FDH_GLYPH_VARIANT_STEPS; g0 < (size_t)base; g0++)
          for (int st = 0; st < FDH_GLYPH_VARIANT_STEPS; st++) variant_ids_.push_back(glyphs_[g0].image_id);
        for (int g = 0; g < f.glyph_count; g++)
          for (int st = 0; st < FDH_GLYPH_VARIANT_STEPS; st++)
            variant_ids_.push_back(side->glyph_variant_ids ? side->glyph_variant_ids[(size_t)(f.glyph_first + g) * FDH_GLYPH_VARIANT_STEPS + st] : side->glyphs[f.glyph_first + g].image_id);
      }
      f.glyph_first = base;
    }
    if (f.text_rect_count > 0) {
      if (!side || !side->text_rects || f.text_rect_first < 0 || f.text_rect_first + f.text_rect_count > side->n_text_rects) throw Error(FDH_ERR_INVALID, "scene update: text-rect range outside the side arrays");
      const int base = (int)text_rects_.size();
      text_rects_.insert(text_rects_.end(), side->text_rects + f.text_rect_first, side->text_rects + f.text_rect_first + f.text_rect_count);
      f.text_rect_first = base;
    }
    if (f.op_count > 0) {
      if (!side || !side->ops || f.op_first < 0 || f.op_first + f.op_count > side->n_ops) throw Error(FDH_ERR_INVALID, "scene update: drawable-op range outside the side arrays");
      const int base = (int)ops_.size();
      for (int k = 0; k < f.op_count; k++) {
        FdhDrawOp op = side->ops[f.op_first + k];
        if (op.ctrl_count > 0) {
          if (!side->controls || op.ctrl_first < 0 || op.ctrl_first + op.ctrl_count > side->n_controls) throw Error(FDH_ERR_INVALID, "scene update: control-point range outside the side arrays");
          const int cb = (int)(controls_.size() / 2);
          controls_.insert(controls_.end(), side->controls + 2 * op.ctrl_first, side->controls + 2 * (op.ctrl_first + op.ctrl_count));
          op.ctrl_first = cb;
        }
        ops_.push_back(op);
      }
      f.op_first = base;
    }
  }
}

// An edit either lands whole or not at all: rebase_side appends to the retained side arrays before it has seen every node of
// the edit, so a bad range found late must take the appended entries back.
struct RetainedScene::SideMark {
  RetainedScene& R;
  const size_t g, v, o, c, t;
  const uint32_t epoch;  // (the first variant table may have appeared with one of the edit's earlier nodes)
  bool keep = false;
  explicit SideMark(RetainedScene& r) : R(r), g(r.glyphs_.size()), v(r.variant_ids_.size()), o(r.ops_.size()), c(r.controls_.size()), t(r.text_rects_.size()), epoch(r.table_epoch_) {}
  ~SideMark() {
    if (keep) return;
    R.glyphs_.resize(g); R.variant_ids_.resize(v); R.ops_.resize(o); R.controls_.resize(c); R.text_rects_.resize(t);
    R.table_epoch_ = epoch;
  }
};

// Every update_nodes / replace_root appends the side entries of the new nodes and orphans those of the old ones; an animated
// text or drawable node would grow the arrays without bound (and n_glyphs past int32).  When the live entries are less than
// half of an array that has grown past a few thousand, the arrays are rebuilt from the nodes that still reference them.  Node
// ranges move, draw records do not depend on them: the per-root caches stay valid.
void RetainedScene::compact_side() {
  size_t live_g = 0, live_o = 0, live_t = 0;
  for (const RetainedLayer& D : layers_)
    for (const FdhFig& f : D.nodes) { live_g += (size_t)std::max(f.glyph_count, 0); live_o += (size_t)std::max(f.op_count, 0); live_t += (size_t)std::max(f.text_rect_count, 0); }
  auto bloated = [](size_t live, size_t have) { return have > 4096 && live * 2 < have; };
  if (!bloated(live_g, glyphs_.size()) && !bloated(live_o, ops_.size()) && !bloated(live_t, text_rects_.size())) return;
  std::vector<FdhGlyph> glyphs;
  std::vector<int64_t> variants;
  std::vector<FdhDrawOp> ops;
  std::vector<float> controls;
  std::vector<FdhTextRect> rects;
  const bool has_var = !variant_ids_.empty();
  for (RetainedLayer& D : layers_)
    for (FdhFig& f : D.nodes) {
      if (f.glyph_count > 0 && f.glyph_first >= 0 && (size_t)f.glyph_first + (size_t)f.glyph_count <= glyphs_.size()) {
        const int base = (int)glyphs.size();
        glyphs.insert(glyphs.end(), glyphs_.begin() + f.glyph_first, glyphs_.begin() + f.glyph_first + f.glyph_count);
        if (has_var)
          for (int g = f.glyph_first; g < f.glyph_first + f.glyph_count; g++)
            for (int st = 0; st < FDH_GLYPH_VARIANT_STEPS; st++) {
              const size_t at = (size_t)g * FDH_GLYPH_VARIANT_STEPS + st;
              variants.push_back(at < variant_ids_.size() ? variant_ids_[at] : glyphs_[(size_t)g].image_id);
            }
        f.glyph_first = base;
      } else if (f.glyph_count > 0) f.glyph_count = 0;
      if (f.text_rect_count > 0 && f.text_rect_first >= 0 && (size_t)f.text_rect_first + (size_t)f.text_rect_count <= text_rects_.size()) {
        const int base = (int)rects.size();
        rects.insert(rects.end(), text_rects_.begin() + f.text_rect_first, text_rects_.begin() + f.text_rect_first + f.text_rect_count);
        f.text_rect_first = base;
      } else if (f.text_rect_count > 0) f.text_rect_count = 0;
      if (f.op_count > 0 && f.op_first >= 0 && (size_t)f.op_first + (size_t)f.op_count <= ops_.size()) {
        const int base = (int)ops.size();
        for (int k = 0; k < f.op_count; k++) {
          FdhDrawOp op = ops_[(size_t)(f.op_first + k)];
          if (op.ctrl_count > 0 && op.ctrl_first >= 0 && 2 * ((size_t)op.ctrl_first + (size_t)op.ctrl_count) <= controls_.size()) {
            const int cb = (int)(controls.size() / 2);
            controls.insert(controls.end(), controls_.begin() + 2 * op.ctrl_first, controls_.begin() + 2 * (op.ctrl_first + op.ctrl_count));
            op.ctrl_first = cb;
          } else op.ctrl_count = 0;
          ops.push_back(op);
        }
        f.op_first = base;
      } else if (f.op_count > 0) f.op_count = 0;
    }
  glyphs_.swap(glyphs); variant_ids_.swap(variants); ops_.swap(ops); controls_.swap(controls); text_rects_.swap(rects);
}

// A retained layer is edited in place (subtrees compacted out, parents remapped): every parent index it holds must be -1 or
// that of an EARLIER node (parents precede their children in a RenderList, fignodes.nim:119-163).
static void check_parents(const FdhFig* nodes, int n, int first_index, const char* who) {
  for (int k = 0; k < n; k++)
    if (nodes[k].parent < -1 || nodes[k].parent >= first_index + k) throw Error(FDH_ERR_INVALID, std::string(who) + ": a node's parent must be -1 or an earlier node of the layer");
}

void RetainedScene::retain(const FdhScene* scene, float fw, float fh, bool clear, const float rgba[4]) {
  if (!scene || (scene->n_layers > 0 && !scene->layers)) throw Error(FDH_ERR_INVALID, "scene_retain: null scene");
  for (int l = 0; l < scene->n_layers; l++) {
    const FdhLayer& L = scene->layers[l];
    if ((L.n_nodes > 0 && !L.nodes) || (L.n_roots > 0 && !L.root_ids)) throw Error(FDH_ERR_INVALID, "scene_retain: a layer's node or root array is null");
    if (L.n_nodes > 32767) throw Error(FDH_ERR_INVALID, "scene_retain: more than 32767 nodes in a layer (FigIdx is int16, fignodes.nim:119)");
    check_parents(L.nodes, L.n_nodes, 0, "scene_retain");
  }
  for (int l = 0; l < scene->n_layers; l++) {
    const FdhLayer& L = scene->layers[l];
    for (int r = 0; r < L.n_roots; r++)
      if (L.root_ids[r] < 0 || L.root_ids[r] >= L.n_nodes) throw Error(FDH_ERR_INVALID, "scene_retain: root index out of range");
  }
  // Everything that can fail has happened: the new scene is built aside and takes the old one's place whole (nothing below throws
  // but std::bad_alloc, and that too leaves the retained scene as it was).
  RetainedScene S;
  S.fw_ = fw; S.fh_ = fh; S.clear_ = clear;
  for (int i = 0; i < 4; i++) S.rgba_[i] = rgba[i];
  if (scene->glyphs && scene->n_glyphs > 0) S.glyphs_.assign(scene->glyphs, scene->glyphs + scene->n_glyphs);
  if (scene->glyph_variant_ids && scene->n_glyphs > 0) S.variant_ids_.assign(scene->glyph_variant_ids, scene->glyph_variant_ids + (size_t)scene->n_glyphs * FDH_GLYPH_VARIANT_STEPS);
  if (scene->ops && scene->n_ops > 0) S.ops_.assign(scene->ops, scene->ops + scene->n_ops);
  if (scene->controls && scene->n_controls > 0) S.controls_.assign(scene->controls, scene->controls + 2 * (size_t)scene->n_controls);
  if (scene->text_rects && scene->n_text_rects > 0) S.text_rects_.assign(scene->text_rects, scene->text_rects + scene->n_text_rects);
  S.layers_.resize((size_t)std::max(scene->n_layers, 0));
  for (int l = 0; l < scene->n_layers; l++) {
    const FdhLayer& L = scene->layers[l];
    RetainedLayer& D = S.layers_[(size_t)l];
    D.zlevel = L.zlevel;
    if (L.n_nodes > 0) D.nodes.assign(L.nodes, L.nodes + L.n_nodes);
    if (L.n_roots > 0) D.roots.assign(L.root_ids, L.root_ids + L.n_roots);
    D.cache.assign(D.roots.size(), RetainedRoot{});
  }
  S.valid_ = true;
  *this = std::move(S);
}

RetainedScene::View RetainedScene::view() const {
  for (const RetainedLayer& D : layers_)
    for (int r : D.roots) if (r < 0 || (size_t)r >= D.nodes.size()) throw Error(FDH_ERR_INVALID, "scene_render: root index out of range");
  View V;
  std::vector<FdhLayer>& views = V.layers;
  views.resize(layers_.size());
  for (size_t l = 0; l < layers_.size(); l++) {
    const RetainedLayer& D = layers_[l];
    views[l] = FdhLayer{D.zlevel, (int32_t)D.nodes.size(), (int32_t)D.roots.size(), 0, D.nodes.data(), D.roots.data()};
  }
  FdhScene& view = V.scene;
  view = FdhScene{};
  view.layers = views.data(); view.n_layers = (int32_t)views.size();
  view.glyphs = glyphs_.data(); view.n_glyphs = (int32_t)glyphs_.size();
  view.glyph_variant_ids = variant_ids_.empty() ? nullptr : variant_ids_.data();
  view.ops = ops_.data(); view.n_ops = (int32_t)ops_.size();
  view.controls = controls_.data(); view.n_controls = (int32_t)(controls_.size() / 2);
  view.text_rects = text_rects_.data(); view.n_text_rects = (int32_t)text_rects_.size();
  return V;
}

// the root (index into the layer's nodes) each node hangs under; parents precede their children in a RenderList (fignodes.nim:119-163)
static std::vector<int> roots_of(const RetainedLayer& D) {
  std::vector<int> ro(D.nodes.size());
  for (size_t i = 0; i < D.nodes.size(); i++) {
    const int p = D.nodes[i].parent;
    ro[i] = (p < 0 || (size_t)p >= i) ? (int)i : ro[(size_t)p];
  }
  return ro;
}

void RetainedScene::update_nodes(int layer, int first, int count, const FdhFig* nodes, const FdhScene* side) {
  if (!valid_) throw Error(FDH_ERR_INVALID, "scene_update_nodes: no retained scene (fdh_scene_retain first)");
  if (layer < 0 || (size_t)layer >= layers_.size()) throw Error(FDH_ERR_INVALID, "scene_update_nodes: layer out of range");
  RetainedLayer& D = layers_[(size_t)layer];
  if (count <= 0) return;
  if (!nodes || first < 0 || (size_t)first + (size_t)count > D.nodes.size()) throw Error(FDH_ERR_INVALID, "scene_update_nodes: node range out of bounds");
  check_parents(nodes, count, first, "scene_update_nodes");
  // the roots above the range before the edit (a node may change its parent) ...
  std::vector<int> before = roots_of(D);
  std::vector<FdhFig> fresh(nodes, nodes + count);
  {
    SideMark mark(*this);  // a bad side range throws out of rebase_side: the entries it had appended go with it
    rebase_side(fresh.data(), count, side);
    mark.keep = true;
  }
  std::copy(fresh.begin(), fresh.end(), D.nodes.begin() + first);
  std::vector<int> after = roots_of(D);  // ... and after it
  for (size_t s = 0; s < D.roots.size(); s++)
    for (int i = first; i < first + count; i++)
      if (before[(size_t)i] == D.roots[s] || after[(size_t)i] == D.roots[s]) { D.cache[s].dirty = true; break; }
  compact_side();
}

void RetainedScene::replace_root(int layer, int slot, const FdhFig* subtree, int n, const FdhScene* side, bool insert) {
  if (!valid_) throw Error(FDH_ERR_INVALID, "scene_replace_root: no retained scene (fdh_scene_retain first)");
  if (layer < 0 || (size_t)layer >= layers_.size()) throw Error(FDH_ERR_INVALID, "scene_replace_root: layer out of range");
  RetainedLayer& D = layers_[(size_t)layer];
  if (slot < 0 || (size_t)slot > D.roots.size() || (!insert && (size_t)slot == D.roots.size())) throw Error(FDH_ERR_INVALID, "scene_replace_root: root slot out of range");
  if (n < 0 || (n > 0 && !subtree)) throw Error(FDH_ERR_INVALID, "scene_replace_root: bad subtree");
  if (n > 0 && subtree[0].parent >= 0) throw Error(FDH_ERR_INVALID, "scene_replace_root: the subtree's first node must be its root (parent -1)");
  for (int i = 1; i < n; i++)
    if (subtree[i].parent < 0 || subtree[i].parent >= i) throw Error(FDH_ERR_INVALID, "scene_replace_root: subtree parents must precede their children");
  // Everything that can fail happens BEFORE the retained layer is touched: the node budget, and the re-basing of the new
  // nodes' side ranges (into a copy; what it appended to the side arrays is taken back if it throws).  A failed call leaves
  // the scene exactly as it was.
  std::vector<int> ro;
  size_t kept_count = D.nodes.size();
  int old_root = -1;
  if (!insert) {
    ro = roots_of(D);
    old_root = D.roots[(size_t)slot];
    kept_count = 0;
    for (size_t i = 0; i < D.nodes.size(); i++) if (ro[i] != old_root) kept_count++;
  }
  if (kept_count + (size_t)n > 32767u) throw Error(FDH_ERR_INVALID, "scene_replace_root: more than 32767 nodes in a layer (FigIdx is int16, fignodes.nim:119)");
  std::vector<FdhFig> fresh;
  if (n > 0) {
    fresh.assign(subtree, subtree + n);
    SideMark mark(*this);
    rebase_side(fresh.data(), n, side);
    mark.keep = true;
  }
  // ---- commit (nothing below throws but std::bad_alloc)
  if (!insert) {  // drop the old subtree, compacting the node array
    std::vector<int> remap(D.nodes.size(), -1);
    std::vector<FdhFig> kept;
    kept.reserve(kept_count + (size_t)n);
    for (size_t i = 0; i < D.nodes.size(); i++)
      if (ro[i] != old_root) { remap[i] = (int)kept.size(); kept.push_back(D.nodes[i]); }
    for (FdhFig& f : kept) if (f.parent >= 0) f.parent = remap[(size_t)f.parent];
    // (the other roots' caches stay clean, and their records' tags name nodes by index: they move with the compaction)
    for (size_t s = 0; s < D.cache.size(); s++)
      if ((int)s != slot)
        for (PickTag& g : D.cache[s].tags) if (g.id >= 0 && (size_t)g.id < remap.size()) g.id = remap[(size_t)g.id];
    // (a root slot whose node hangs inside the removed subtree -- fdh_scene_update_nodes may have given a listed root a parent --
    // goes with it: it would name a node that no longer exists)
    for (size_t s = D.roots.size(); s-- > 0;) {
      if ((int)s == slot) continue;
      const int to = remap[(size_t)D.roots[s]];
      if (to >= 0) { D.roots[s] = to; continue; }
      D.roots.erase(D.roots.begin() + (std::ptrdiff_t)s);
      D.cache.erase(D.cache.begin() + (std::ptrdiff_t)s);
      if ((int)s < slot) slot--;
    }
    D.nodes.swap(kept);
    if (n == 0) { D.roots.erase(D.roots.begin() + slot); D.cache.erase(D.cache.begin() + slot); compact_side(); return; }
  } else {
    if (n == 0) return;
    D.roots.insert(D.roots.begin() + slot, 0);
    D.cache.insert(D.cache.begin() + slot, RetainedRoot{});
  }
  const int base = (int)D.nodes.size();
  for (int i = 1; i < n; i++) fresh[(size_t)i].parent += base;
  D.nodes.insert(D.nodes.end(), fresh.begin(), fresh.end());
  D.roots[(size_t)slot] = base;
  D.cache[(size_t)slot] = RetainedRoot{};
  compact_side();
}

}  // namespace fdh
