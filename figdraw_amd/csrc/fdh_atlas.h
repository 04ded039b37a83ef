// fdh_atlas.h -- the image atlas (fdh_atlas.cpp): the directory of entries, the skyline packer and the level chains in device memory: one
// member of Context.  The context quiesces its stream (a frame in flight may sample the atlas) and hands it over with every call; the
// atlas does not know the context.  Glyphs made on the device are GlyphMaker's (fdh_glyphs.h), which places them here.
#pragma once
#include <cstdint>
#include <memory>
#include <unordered_map>
#include <vector>

#include "../../include_glyphs/figdraw_hip_atlas.h"  // FdhAtlasMoveStats, FdhAtlasUsage
#include "fdh_memory.h"  // hipStream_t
#include "fdh_types.h"   // AtlasView, kMaxMips

namespace fdh {

// An atlas entry and, when its level-0 texels were seen on the host (fdh_put_image), the bounds of what is IN it: for eight
// levels t = 0, 16, .. 112 the box (entry-relative texels, x1 / y1 exclusive) of texels whose alpha, and whose largest colour
// channel, exceeds t.  A draw whose coverage is exactly 0 wherever the sampled value is <= t (a glyph image: alpha 0; an MSDF
// image: distance below threshold - 0.5 / screen range) shrinks its pixel bounds to the image of that box: the strips outside
// would blend with alpha 0, which leaves every texel as it is (Recorder::shrink_to_ink).
constexpr int kInkLevels = 8;
struct InkBox { int16_t x0, y0, x1, y1; };
// What an entry's put stored, which a move of the entry (Atlas::compact) has to know.  Every level rectangle lies at (x >> l, y >> l):
// - chain: the level chain of updateSubImage, ceil(w / 2^l) x ceil(h / 2^l) while both exceed 1 (each_level) -- nothing of an image 1 texel
//   wide or high;  chain_or_level0: the same, and level 0 alone of such an image (a distance field: GlyphMaker::put_field);
// - levels: the caller's own levels (put_mips, put_flippy), of sizes that need not be the chain's; a rectangle that leaves its level was
//   not stored (upload_rect).  Levels 1 .. of such an entry are kept on the host: where a neighbour's put has overwritten a shared texel
//   since, the atlas no longer holds them.
enum class Stored : uint8_t { chain, chain_or_level0, levels };
struct KeptLevels {
  int n = 0;
  int w[kMaxMips] = {}, h[kMaxMips] = {};
  std::vector<uint32_t> texels;  // of levels 1 .. n - 1, one after the other, rows packed
};
struct AtlasEntry {
  int x, y, w, h;
  bool has_ink = false;
  InkBox ink_a[kInkLevels], ink_rgb[kInkLevels];
  Stored stored = Stored::chain;
  std::shared_ptr<const KeptLevels> kept;  // Stored::levels only
};
// the level rectangles of `e` in an atlas of `size` with n_levels levels: step(level, x, y, w, h), level 0 first
template <typename Step> void each_stored(const AtlasEntry& e, int size, int n_levels, Step step) {
  if (e.stored == Stored::levels) {
    for (int l = 0; e.kept && l < e.kept->n && l < n_levels; l++) {
      const int LS = size >> l, x = e.x >> l, y = e.y >> l, w = e.kept->w[l], h = e.kept->h[l];
      if (x + w <= LS && y + h <= LS) step(l, x, y, w, h);
    }
    return;
  }
  if (e.stored == Stored::chain_or_level0 && (e.w == 1 || e.h == 1)) { step(0, e.x, e.y, e.w, e.h); return; }
  int x = e.x, y = e.y, w = e.w, h = e.h;
  for (int l = 0; w > 1 && h > 1 && l < n_levels; l++, x /= 2, y /= 2, w = (w + 1) / 2, h = (h + 1) / 2) step(l, x, y, w, h);
}

class Atlas;
// Who moves the texels when the atlas is compacted (GlyphMaker: the scratch buffers and the level chain's kernels are its).  `moved`: the
// live entries in compaction order, as they lie in the new atlas, and where each lay in the old one; `to` has its new levels (cleared),
// size and level count, and still its old directory.  Waits for the stream before it returns.
struct MovedEntry { const AtlasEntry* e; int old_x, old_y; };
struct AtlasMover {
  virtual void move_entries(hipStream_t s, const AtlasView& from, const Atlas& to, const std::vector<MovedEntry>& moved, FdhAtlasMoveStats& stats) = 0;
 protected:
  ~AtlasMover() = default;
};

class Atlas {
 public:
  // ---- directory and packer: no device needed (a record-only context has both)
  void init(int size, bool device, hipStream_t s);  // a context's first atlas; `device`: the levels exist (else only the directory and the packer)
  const AtlasEntry* find(int64_t key) const {       // (the walk pool's threads call this while they record)
    auto it = entries_.find(key);
    return it == entries_.end() ? nullptr : &it->second;
  }
  bool has(int64_t key) const { return entries_.count(key) != 0; }
  void remove(int64_t key) { entries_.erase(key); epoch_++; }
  int size() const { return size_; }
  int n_levels() const { return n_levels_; }
  // moves with every put, update, remove and reset: cached draw records of image nodes carry atlas positions (RetainedRoot::atlas_epoch)
  uint64_t epoch() const { return epoch_; }
  int64_t packed_area() const;
  void reset(int minimum_size, hipStream_t s);
  // ---- compaction and keep mode (the specification: include_glyphs/figdraw_hip_atlas.h)
  void set_mover(AtlasMover* m) { mover_ = m; }
  void compact(hipStream_t s, int size, FdhAtlasMoveStats* out);
  void set_keep(bool on) { keep_ = on; }
  bool keep() const { return keep_; }
  // in front of a placement: in keep mode, where the n images (w, h) do not all fit the atlas as it stands, compact it to the smallest
  // size that takes the live entries and these images (or to 16384); nothing otherwise
  void make_room(hipStream_t s, const int (*wh)[2], int n);
  void make_room(hipStream_t s, int w, int h) { const int one[1][2] = {{w, h}}; make_room(s, one, 1); }
  void usage(FdhAtlasUsage* out) const;
  // ---- what the kernels sample, and level 0 for fdh_debug_read_surface
  AtlasView view() const;
  const uint32_t* level0() const { return levels_[0]; }
  // ---- what a put from outside (GlyphMaker, Importer) needs: THE placement -- rect (growing as needed, which drops every entry), entry, epoch,
  // out_rect; whether the levels exist; a level's texels (valid until the next placement); and updateSubImage's level chain
  // (textures.nim:106-119): step(level, x, y, w, h) for the image minified `level` times, while width > 1 and height > 1
  // `stored`: what the put will store of the image (AtlasEntry::stored); put_mips sets its own
  AtlasEntry& place(hipStream_t s, int64_t key, int w, int h, int out_rect[4], Stored stored = Stored::chain);
  bool has_device() const { return device_; }
  uint32_t* level(int l) const { return levels_[l]; }
  template <typename Step> void each_level(int x, int y, int w, int h, Step step) const {
    for (int level = 0; w > 1 && h > 1 && level < n_levels_; level++, x /= 2, y /= 2, w = (w + 1) / 2, h = (h + 1) / 2) step(level, x, y, w, h);
  }
  // ---- texel work.  Every put validates and only then takes a place: one that throws before its texels are on their way leaves no
  // entry and no epoch bump behind.
  void put_image(hipStream_t s, int64_t key, int w, int h, const uint8_t* rgba, int out_rect[4]);
  void put_mips(hipStream_t s, int64_t key, int n, const int* ws, const int* hs, const uint8_t* const* premul_rgba, int out_rect[4]);
  void put_flippy(hipStream_t s, int64_t key, const uint8_t* data, size_t n, int out_rect[4]);
  void update_image(int64_t key, int w, int h, const uint8_t* rgba);
  // the first half of every update, the host's and the Importer's from device memory: the key is looked up, the size checked, the epoch
  // bumped, an entry with levels of its own turned into a chain entry; the caller stores the new chain and the ink boxes
  AtlasEntry& begin_update(const char* who, int64_t key, int w, int h, const char* also_refused = nullptr);
  void release() { release_levels(); }  // (the stream is idle)

 private:
  void alloc(int size, hipStream_t s);  // new levels first, then the old ones go and the empty atlas is committed
  int alloc_levels(int sz, hipStream_t s, uint32_t* fresh[kMaxMips]) const;  // the cleared levels of an atlas of sz (a power of two); -> their number
  // THE skyline search (glcontext.nim:541-579) on any skyline of S columns: the place of a w x h image, its columns raised; false: no room
  static bool skyline_place(std::vector<uint16_t>& heights, int S, int margin, int w, int h, int* x, int* y);
  std::vector<const std::pair<const int64_t, AtlasEntry>*> compaction_order() const;
  void release_levels();
  void upload_rect(int level, int x, int y, int w, int h, const uint8_t* rgba);
  void put_levels(int x, int y, int w, int h, const uint8_t* rgba);

  bool device_ = false;
  int size_ = 0, initial_size_ = 0, margin_ = 4, n_levels_ = 0;
  uint32_t* levels_[kMaxMips] = {};
  std::vector<uint16_t> heights_;  // the skyline
  std::unordered_map<int64_t, AtlasEntry> entries_;
  uint64_t epoch_ = 1;
  bool keep_ = false;
  int64_t rebuilds_ = 0, compactions_ = 0;
  AtlasMover* mover_ = nullptr;
};

}  // namespace fdh
