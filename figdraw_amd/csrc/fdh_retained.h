// fdh_retained.h -- the retained scene (fdh_retained.cpp): the tree fdh_scene_retain copied, the side arrays its nodes index, and per
// root the draw records of its last decomposition: one member of Context.  It edits and describes the tree; it records nothing and
// knows neither the context nor a device (plain C++: fdh_plain.h is all it needs).  Context::scene_render walks what view() shows.
#pragma once
#include <cstdint>
#include <vector>

#include "fdh_plain.h"

namespace fdh {

// Retained scene (fdh_scene_*): the library-side half of the reference's RenderFragments (renderfragments.nim:426-544) --
// a deep copy of the node tree plus, per root, the draw records its decomposition produced.  A frame re-decomposes only the
// roots an update touched; every other root's records are spliced back from the cache.
struct RetainedRoot {
  std::vector<DrawRec> recs;     // in device form (Recorder::push_rec)
  std::vector<BinRec> bins;      // bounds, cores, list-entry flags (the last record's LE_SHARE is decided again at every splice)
  std::vector<QuadExt> exts;     // of this root's records, DrawRec::ext relative to exts.front()
  std::vector<PickTag> tags;     // of this root's records, when it was walked in a picking frame (tagged)
  bool tagged = false;
  PhaseSum sum;
  int64_t fragments = 0;
  bool cacheable = false;        // no blur node inside (those split the frame into phases: re-walked every frame)
  bool dirty = true;
  uint64_t atlas_epoch = 0;      // image draws carry atlas positions: stale after the atlas was rebuilt
  int cull_y0 = 0, cull_y1 = 0;  // the rows the records were culled to (Context::begin_frame)
};
struct RetainedLayer {
  int32_t zlevel = 0;
  std::vector<FdhFig> nodes;
  std::vector<int32_t> roots;
  std::vector<RetainedRoot> cache;  // parallel to `roots`
};

class RetainedScene {
 public:
  // ---- edits (fdh_scene_retain / _update_nodes / _replace_root / _insert_root).  Each lands whole or not at all: one that throws
  // leaves the scene -- after a failed retain, the previously retained one -- exactly as it was.
  void retain(const FdhScene* scene, float fw, float fh, bool clear, const float rgba[4]);
  void update_nodes(int layer, int first, int count, const FdhFig* nodes, const FdhScene* side);
  void replace_root(int layer, int slot, const FdhFig* subtree, int n, const FdhScene* side, bool insert);

  // ---- what a frame of it needs (Context::scene_render)
  bool valid() const { return valid_; }
  float fw() const { return fw_; }
  float fh() const { return fh_; }
  bool clear() const { return clear_; }
  const float* rgba() const { return rgba_; }
  // the tree as the scene front-end reads one, over the retained storage: layer l of it is layer(l)'s nodes and roots.  Good until
  // the next edit.
  struct View { std::vector<FdhLayer> layers; FdhScene scene; };  // (scene.layers is layers.data())
  View view() const;
  // every cached record depends on these front-end settings (the text path snaps glyph positions and picks shifts / variant
  // images by the two sub-pixel switches, figrender.nim:464-476): did one of them -- or the glyph-variant table's presence -- change
  // since the last call?  Records the new values.
  bool latch_settings(float ui_scale, float aa, bool subpixel, bool variants) {
    const bool changed = ui_scale_ != ui_scale || aa_ != aa || subpixel_ != subpixel || variants_ != variants || table_epoch_ != table_epoch_seen_;
    ui_scale_ = ui_scale; aa_ = aa; subpixel_ = subpixel; variants_ = variants; table_epoch_seen_ = table_epoch_;
    return changed;
  }
  size_t n_layers() const { return layers_.size(); }
  const RetainedLayer& layer(size_t l) const { return layers_[l]; }
  RetainedRoot& cache(size_t l, size_t slot) { return layers_[l].cache[slot]; }  // of root layer(l).roots[slot]
  // roots decomposed / spliced back from their cache by the last fdh_scene_render (Context::scene_render counts them)
  void count_begin() { roots_walked_ = roots_reused_ = 0; }
  void count_walked() { roots_walked_++; }
  void count_reused() { roots_reused_++; }
  void stats(int64_t* walked, int64_t* reused) const { *walked = roots_walked_; *reused = roots_reused_; }

 private:
  struct SideMark;
  void rebase_side(FdhFig* nodes, int n, const FdhScene* side);
  void compact_side();

  bool valid_ = false;
  float fw_ = 0, fh_ = 0, rgba_[4] = {1, 1, 1, 1};
  bool clear_ = true;
  float ui_scale_ = 1.0f, aa_ = 0.0f;
  bool subpixel_ = false, variants_ = false;  // the text front-end settings the cached records were made under
  uint32_t table_epoch_ = 0, table_epoch_seen_ = 0;  // bumped when a glyph-variant table first appears (rebase_side)
  std::vector<RetainedLayer> layers_;
  std::vector<FdhGlyph> glyphs_;
  std::vector<int64_t> variant_ids_;  // [glyphs][FDH_GLYPH_VARIANT_STEPS] or empty
  std::vector<FdhDrawOp> ops_;
  std::vector<float> controls_;
  std::vector<FdhTextRect> text_rects_;
  int64_t roots_walked_ = 0, roots_reused_ = 0;  // of the last fdh_scene_render
};

}  // namespace fdh
