// fdh_import.h -- images and decoded video frames from device memory into the atlas (fdh_import.cpp): class Importer, one member of Context
// beside the atlas and the glyph maker.  A source -- an FdhDeviceImage, an FdhVideoFrame, three or four video planes, or a batch of the first
// two -- is validated, gets its scratch buffers and only then a place in the atlas (Atlas::place, Atlas::begin_update); kernels on the stream
// the context hands over with every call convert it and make the atlas's level chain and the entry's ink boxes.  The importer knows neither
// the context nor how the atlas packs, and its scratch is its own: it shares no buffer with GlyphMaker.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include_glyphs/figdraw_hip_device_images.h"  // FdhImageBatchStats; and through it figdraw_hip_device_image.h (FdhDeviceImage)
#include "../../include_glyphs/figdraw_hip_video_frames.h"  // FdhVideoBatchStats; and through it figdraw_hip_video_frame.h (FdhVideoFrame)
#include "../../include_video/figdraw_hip_video_alpha.h"    // FdhVideoAlphaPlanes; through it figdraw_hip_video_422.h (the 4:2:2 formats) and
                                                            // figdraw_hip_video_planar.h (FdhVideoPlanes)
#include "fdh_atlas.h"
#include "fdh_memory.h"  // DeviceBuf, PinnedBuf

namespace fdh {

class Importer final {
 public:
  // Every call asks in this order: the struct's own rules; an update's key and size ("unknown key", "size mismatch"); on a context with a
  // device the pointers, then the buffers; and only then takes its place.  One that throws before its texels are on their way leaves no entry
  // and no epoch bump behind.  Each waits for the stream once, at its end.  `device`: the context's (a record-only context asks nothing of it).
  // fdh_put_image_device and fdh_update_image_device (the specification: include_glyphs/figdraw_hip_device_image.h): what Atlas::put_image and
  // Atlas::update_image store, of a source in device memory
  void put_device_image(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhDeviceImage* img, int out_rect[4]);
  void update_device_image(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhDeviceImage* img);
  // fdh_put_images_device and fdh_update_images_device (the specification: include_glyphs/figdraw_hip_device_images.h): n device images, validated
  // as a whole, placed (their updates begun) in order, made in at most four launches
  void put_device_images(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n, int (*out_rects)[4]);
  void update_device_images(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhDeviceImage* images, int n);
  const FdhImageBatchStats& image_batch_stats() const { return image_stats_; }
  // fdh_put_video_frame and fdh_update_video_frame (the specification: include_glyphs/figdraw_hip_video_frame.h): the same of an NV12, P010 or
  // BGRA8 frame
  void put_video_frame(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoFrame* frame, int out_rect[4]);
  void update_video_frame(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoFrame* frame);
  // fdh_put_video_frames and fdh_update_video_frames (the specification: include_glyphs/figdraw_hip_video_frames.h): n such frames, validated as a
  // whole, placed (their updates begun) in order, made in at most six launches
  void put_video_frames(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n, int (*out_rects)[4]);
  void update_video_frames(hipStream_t s, Atlas& atlas, int device, const int64_t* keys, const FdhVideoFrame* frames, int n);
  const FdhVideoBatchStats& video_batch_stats() const { return video_stats_; }
  // fdh_put_video_planes and fdh_update_video_planes (the specification: include_video/figdraw_hip_video_planar.h): the same of a three-plane
  // I420, I010, I444 or I410 frame
  void put_video_planes(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]);
  void update_video_planes(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame);
  // fdh_put_video_422 and fdh_update_video_422 (the specification: include_video/figdraw_hip_video_422.h): the same of a 4:2:2 frame, I422 or
  // I210 in three planes, YUY2 or UYVY in one
  void put_video_422(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame, int out_rect[4]);
  void update_video_422(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoPlanes* frame);
  // fdh_put_video_alpha and fdh_update_video_alpha (the specification: include_video/figdraw_hip_video_alpha.h): the same of a frame with an
  // alpha plane, A420, A444 or A410 in four planes, UYVA in two
  void put_video_alpha(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoAlphaPlanes* frame, int out_rect[4]);
  void update_video_alpha(hipStream_t s, Atlas& atlas, int device, int64_t key, const FdhVideoAlphaPlanes* frame);
  void release();  // the scratch buffers (the stream is idle)

 private:
  // the ten single calls: `who` names the caller, Source (fdh_import.cpp) is its family -- the struct's rules, its planes on the device, its first kernel
  template <typename Source, typename Struct>
  void import_one(const char* who, bool update, hipStream_t s, Atlas& atlas, int device, int64_t key, const Struct* given, int out_rect[4]);
  void reserve_import(int w, int h);
  // behind the first launch of any of them: the rest of the chain from the level-5 image in level5_, the wait, the entry's ink boxes
  void finish_import(hipStream_t s, const Atlas& atlas, AtlasEntry& e, int n_store);
  // the four batch calls: pass 1 of each kind (fdh_import.cpp), then the buffers, the places (the updates begun) and pass 3 of either kind;
  // pass 3 -- the tables, the launches, the wait, the ink boxes -- of entries first .. first + m - 1
  struct ImageBatch;
  struct VideoBatch;
  template <typename Batch> void reserve_batch(const Batch& B);
  template <typename Batch, typename Stats> void put_batch(hipStream_t s, Atlas& atlas, const int64_t* keys, int n, int (*out_rects)[4], Batch& B, Stats& stats);
  template <typename Batch, typename Stats> void update_batch(const char* who, hipStream_t s, Atlas& atlas, const int64_t* keys, int n, Batch& B, Stats& stats);
  void make(hipStream_t s, const Atlas& atlas, ImageBatch& B, int first, int m);
  void make(hipStream_t s, const Atlas& atlas, VideoBatch& B, int first, int m);

  DeviceBuf<uint32_t> level5_, minified_;  // a single import's level-5 image (a batch: a texel per tile) and what k_minify2 makes of it
  DeviceBuf<uint32_t> tab_;                // the batches: the records, the tile words, the owner bits of the deep levels (fdh_image_batch.h, fdh_video_batch.h)
  PinnedBuf<int32_t> ink_host_;            // the tiles' ink blocks, which the kernels store into page-locked memory (fdh_image_import.h)
  FdhImageBatchStats image_stats_ = {};    // of the last put_device_images or update_device_images
  FdhVideoBatchStats video_stats_ = {};    // of the last put_video_frames or update_video_frames
};

// fdh_video_coefficients (include_glyphs/figdraw_hip_video_frame.h): a row of video_import::kCoefficients; no context
void video_coefficients(uint32_t format, uint32_t matrix, uint32_t range, int32_t out[7]);

}  // namespace fdh
