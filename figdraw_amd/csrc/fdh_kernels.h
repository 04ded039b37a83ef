// fdh_kernels.h -- kernel parameter blocks and launchers shared by the kernel units (k_*.hip) and the host context.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

#include "fdh_types.h"

namespace fdh {

struct BinParams {
  const BinRec* binrec;  // per draw: clipped pixel bounds (ops that must reach every tile carry the frame), saturated core, entry flags
  const uint32_t* binbox; // per draw: x0 | y0 << 8 | (127 - x1) << 16 | (127 - y1) << 24 in (64 << binbox_shift)-px units, padded to 4 draws
  const uint32_t* chunkbox;  // per 256 draws: byte-wise min of their bin boxes = the union box, same format
  int n_draws, binbox_shift;
  uint2* lists;         // [phase][bin][stride] entries {draw index, 16-bit strip mask}
  uint32_t* counts;     // [phase][bin]
  const int* phase_first;  // [n_phases + 1]
  int n_phases, bins_x, bins_y, stride;
  const DrawRec* draws;    // the frame's records: the bin kernel pulls them into every XCD's L2 for the compositor (see k_bin_draws)
  const QuadExt* exts;     // the edge functions of rotated quads (BR_GENERAL draws: strips outside the quad are dropped from the entry)
  int refine;              // the frame holds BR_GENERAL / BR_CURVE draws: the build of k_bin_draws with their per-strip tests
  uint32_t* seq_out = nullptr;  // pinned host word that receives `seq` when the launch starts (or null): see k_bin_draws
  uint32_t seq = 0;
  // Bins per phase: phase p's workgroups are sub_first[p] .. sub_first[p + 1] - 1 and cover the sub_nx[p] bins wide block at
  // (sub_x0[p], sub_y0[p]) -- what that phase's compositor launch will read (a later phase touches the bins of ITS draws; a
  // workgroup per bin of the whole grid for every phase was two thirds of the bench frame's bin launch doing nothing).
  // sub_n = 0: more than kBinSubs phases, every phase gets the whole grid.
  static constexpr int kBinSubs = 8;
  int sub_n = 0;
  int sub_first[kBinSubs + 1] = {};
  int sub_x0[kBinSubs] = {}, sub_y0[kBinSubs] = {}, sub_nx[kBinSubs] = {};
};

struct CompositeParams {
  // (what a wave needs first comes first: with kernel-argument preloading the leading dwords arrive in SGPRs with the wave)
  const int* order;         // bins of a full-grid launch sorted by list length, longest first, or null (built by the
                            // previous frame's launch)
  int* order_next;          // if set, one extra wavefront of this launch sorts this frame's counts into it
  const uint32_t* counts;  // this phase's [bin]
  const uint2* lists;      // this phase's [bin][stride]
  int bin_x0, bin_y0, bin_nx, bin_ny;  // sub-grid of bins this launch covers
  int bins_x, stride;
  int row_lo, row_hi;       // stripe: only rows in [row_lo,row_hi) are produced
  int W, H, pitch;          // pitch in pixels
  int load_fb;              // 0: start from clear_rgba8
  uint32_t clear_rgba8;
  int n_wg;                 // total workgroups (for the XCD remap)
  uint32_t* fb;
  const uint32_t* backdrop;  // blurred snapshot sampled by mode 17
  int has_masks;            // the phase holds clip / rect-mask ops (disables per-strip occlusion culling)
  int has_slow;             // the phase holds draws that need the one-pixel-slot path (k_composite_tiles<3>)
  int has_slow_atlas = 0;   // ... atlas quads among them: k_composite_tiles<19>, the same build at three waves per SIMD (168 registers)
  int has_rot;              // ... or rotated SDF quads the 4-wide path takes (k_composite_tiles<8>, or <3> with the others)
  int has_atlas;            // ... or axis-aligned atlas quads at >= 1:1 (k_composite_tiles<2>)
  // block waves (blocks::k_composite_tiles): the positions of `order` from block_k8 on (a multiple of 8) get one wave per
  // 32 x 32 block, those in front of it one per strip; < 0: the launch must not take the form.  (In the four bytes that were padding in
  // front of `mask_spill`, as block_max below sits in those in front of `binrec`: the block keeps its size and every field its place.)
  int block_k8 = -1;
  uint32_t* mask_spill;     // clip-stack levels beyond kMaskDepth: [level - kMaskDepth][strip][lane] (null when no frame nests that deep)
  size_t spill_stride;      // dwords per level = strips of the frame x 64
  AtlasView atlas;
  // quarter strips (round 6, k_composite_tiles): the first deep_k8 positions of `order` (a multiple of 8) are shaded by four waves per
  // strip; deep_min / deep_out: the sorting waves count the bins with at least deep_min draws per class into deep_out[0..7]
  // (pinned host memory, or null)
  // a direct launch (round 6): the phase has at most 64 draws and no list -- the compositor's waves make their bin's entries themselves
  // from the bin records of draws [direct_first, direct_first + direct_n)
  int direct = 0, direct_first = 0, direct_n = 0;
  // block waves: the sorting waves also count the bins with MORE than block_max draws per class, into deep_out[8..15] (0: they do not) --
  // the next launches' block_k8
  int block_max = 0;
  const BinRec* binrec = nullptr;
  int deep_k8 = 0;
  int deep_strip_min = 0;   // ... those of their strips that have at least this many draws to SHADE (strip_shade_count); the others keep their one wave
  int deep_min = 0;
  // the surface is opaque when the launch starts and stays so (LaunchJob::opaque: a cleared frame whose folded clear colour has alpha 255):
  // composite_build may take a build that does not carry the alpha lane, k_composite_tiles<4 | 32>.  (In the four bytes that were padding
  // in front of `deep_out`: the block keeps its size and every field its place -- the builds that hold it in scratch keep their frames.)
  int opaque = 0;
  uint32_t* deep_out = nullptr;
};
static_assert(offsetof(CompositeParams, deep_out) == offsetof(CompositeParams, opaque) + 4 && offsetof(CompositeParams, deep_out) + 8 == sizeof(CompositeParams), "`opaque` sits in what was padding");
static_assert(offsetof(CompositeParams, mask_spill) == offsetof(CompositeParams, block_k8) + 4 && offsetof(CompositeParams, binrec) == offsetof(CompositeParams, block_max) + 4 &&
              sizeof(CompositeParams) == 312, "`block_k8` and `block_max` sit in what was padding");

struct BlurParams {
  const uint32_t* src;
  uint32_t* dst;
  int W, H, pitch;
  int x0, y0, x1, y1;  // output region
  // V pass only: when fuse_draw >= 0 the mode-17 quad that consumes this blur is composited straight into
  // `dst` (the live surface) instead of writing the blurred snapshot out and reading it back
  int fuse_draw;
  // Toeplitz weight fragments of this pass for k_blur_mx (Context::submit builds them: [k-step][hi, lo][lane] x 8 halves),
  // or null: the packed-FMA passes then take the launch
  const uint4* mx_w;
  BlurTaps taps;
  // pixels of the NODE's whole footprint (0: of this launch's region): which passes take the launch -- matrix pipe or VALU -- goes by
  // it, so that a row stripe of a large node runs the kernels the whole frame runs (their sums differ in the last bits)
  long long node_pixels = 0;
  // every texel the pass reads has alpha 255 (an opaque frame's surface, or the H pass's output of one) and the weight fragments sum to
  // the scale closely enough that the filtered alpha rounds to 255 (kMxOpaqueSumBound): the matrix-pipe kernels then filter three
  // channels and write the constant.  The VALU passes do not look at it.
  int opaque = 0;
};

// profile mode: the next launch_* call stamps these events with its kernel's own start / end (nullptr: plain launches)
void set_launch_events(hipEvent_t start, hipEvent_t stop);
bool launch_events_used();
void launch_bin(hipStream_t s, const BinParams& P);
// FDH_FORCE_KERNEL_PATHS=1|2|3|8|19 (a test hook, tests/test_hip_parity.py: every build must give the same pixels): compositor launches on
// a more general build than their phase needs -- <0> with clip masks, <2>, <3>, <8>, <3> at 168 registers <19> (composite_build)
inline int forced_kernel_paths() { static const int v = [] { const char* e = std::getenv("FDH_FORCE_KERNEL_PATHS"); return e ? std::atoi(e) : 0; }(); return v; }
// What a compositor launch of P takes (k_composite.hip): the build k_composite_tiles<paths> / k_composite_damage<paths>, its dynamic LDS
// bytes, and the deep strips -- P.deep_k8 (a multiple of 8, at most the launch's bins rounded up to 8) where the launch can have them: the
// full-frame launch of build <4> with both order pointers, then k_composite_deep's (deep); 0 elsewhere.  Applies FDH_FORCE_KERNEL_PATHS
// to P's phase flags first (the kernels read them).
// block: the full-frame launch of <4> / <4 | 32> takes the block-wave form, block_k8 = where in `order` its four-strip waves begin
// (at most the launch's bins rounded up to 8: then no bin has them)
struct CompositeBuild { int paths = 4; size_t lds = 0; int deep_k8 = 0; bool deep = false; bool block = false; int block_k8 = 0; };  // (paths: 4 | 32 = <4> for an opaque surface)
CompositeBuild composite_build(CompositeParams& P);
void launch_composite(hipStream_t s, const DrawRec* draws, const QuadExt* exts, CompositeParams P);
void launch_blur_h(hipStream_t s, const BlurParams& P);
void launch_blur_v(hipStream_t s, const BlurParams& P, const DrawRec* draws, const QuadExt* exts);
// a small region (blur_one_kernel_ok): both passes in ONE kernel, P.src -> the blurred snapshot in P.dst (out of place: the backdrop
// surface), rows [P.y0, P.y1) of columns [P.x0, P.x1); the phase's compositor launch samples it for the mode-17 quad
bool blur_one_kernel_ok(int w, int h, int reach);
void launch_blur_small(hipStream_t s, const BlurParams& P);
// both passes of a full-frame node in one kernel, out of place (P.src -> P.dst, the fused mode-17 composite blended over P.src);
// P.mx_w = the horizontal pass's weight fragments, w_v = the vertical pass's.  false: no instantiation for this filter width
bool blur_fused_supported(int reach, int W, int pitch);
bool launch_blur_fused(hipStream_t s, const BlurParams& P, const uint4* w_v, const DrawRec* draws, const QuadExt* exts);
void launch_fill(hipStream_t s, uint32_t* p, uint32_t v, size_t n);
// glyph images: LCD filter (pixie_raster.nim:12-43), one minifyBy2 step, copy into an atlas level
// glyph outline (flattened to lines x0, y0, x1, y1) -> premultiplied white coverage; scratch: h x (w + 2) floats
void launch_rasterize_lines(hipStream_t s, const float4* lines, int n, int w, int h, float* scratch, uint32_t* out);
void launch_lcd_filter(hipStream_t s, const uint32_t* src, uint32_t* dst, int w, int h);
void launch_minify2(hipStream_t s, const uint32_t* src, uint32_t* dst, int sw, int sh);  // dst: ((sw + 1) / 2) x ((sh + 1) / 2)
void launch_atlas_blit(hipStream_t s, uint32_t* level, int LS, int x, int y, const uint32_t* src, int w, int h);
// distance-field generation (k_msdf.hip): n_edges records of msdf::kEdgeFloats floats (fdh_msdf_host.h) -> a w x h RGBA8 image, R, G, B the
// channels' signed pseudo-distances, A the true signed distance, each 0.5 + d / range in 8 bits; orient = the sign of the outline's area
void launch_msdf_generate(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, uint32_t* out);
// step 5 of the same specification, the correction pass of FDH_GLYPH_MTSDF_CORRECT (k_msdf_correct): the generated image `in` -> `out` (another
// buffer: every decision reads `in`), same edge records; a texel convicted of carrying a false median between itself and a neighbour gets R = G = B = median
void launch_msdf_correct(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, const uint32_t* in, uint32_t* out);
// step 6, FDH_GLYPH_MTSDF_OVERLAP: the two launches above with the contours combined (k_msdf_generate_union, k_msdf_correct_union); the
// records are the same, slot 15 of a contour's last one says where it ends and whether it is filled (+1) or a hole (-1)
void launch_msdf_generate_union(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, uint32_t* out);
void launch_msdf_correct_union(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, const uint32_t* in, uint32_t* out);
// fdh_put_glyph_outline_cubic (include_glyphs/figdraw_hip_cubic.h; k_msdf_cubic.hip): launch_msdf_generate and launch_msdf_correct for an outline
// that holds cubic segments -- n_edges records of msdf::cubic::kCubicEdgeFloats floats (fdh_msdf_cubic_host.h): lines, quadratics and cubics
void launch_msdf_generate_cubic(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, uint32_t* out);
void launch_msdf_correct_cubic(hipStream_t s, const float* edges, int n_edges, int w, int h, float orient, float range, const uint32_t* in, uint32_t* out);
// fdh_put_glyph_outlines (include_glyphs/figdraw_hip_glyphs.h): the launches above and the level chain for a batch of glyphs at once.  `glyphs`: one
// msdf::BatchGlyph each (fdh_msdf_host.h); `tile_glyph`: the glyph of each of the n_tiles 8 x 8 tiles, the 1-D grid of every launch here; the
// edge records of all glyphs in `edges`, their fields one after the other in `out` / `in` / `src` / `dst`.  `overlap`: step 6's kernels.
// Level l of the chain: the blit of every glyph that has that level (`owner`: one bit per texel from level msdf::kOwnerLevel on, set
// where the glyph is the last of the batch to cover the texel), and its minify from `src` into `dst`.
namespace msdf { struct BatchGlyph; }
void launch_msdf_generate_batch(hipStream_t s, bool overlap, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, uint32_t* out);
void launch_msdf_correct_batch(hipStream_t s, bool overlap, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* in,
                               uint32_t* out);
// fdh_put_glyph_outlines_cubic (include_glyphs/figdraw_hip_cubic_batch.h; k_msdf_cubic.hip): the two launches above over records of
// msdf::cubic::kCubicEdgeFloats floats, in which a glyph's edge_off counts.  (No `overlap`: step 6 takes no cubic.)
void launch_msdf_generate_cubic_batch(hipStream_t s, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, uint32_t* out);
void launch_msdf_correct_cubic_batch(hipStream_t s, const float* edges, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* in,
                                     uint32_t* out);
void launch_atlas_blit_batch(hipStream_t s, uint32_t* level, int LS, int l, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* owner,
                             const uint32_t* src);
void launch_minify2_batch(hipStream_t s, int l, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* src, uint32_t* dst);
// fdh_put_glyph_coverage_batch (include_glyphs/figdraw_hip_coverage.h): the coverage of every glyph of a batch, over the same tables -- a glyph's edge_off /
// n_edges are its first flattened line (x0, y0, x1, y1) in `lines` and its line count.  Two launches: the area cells of all tiles into
// `acc` (floats, laid out like the fields: the spare field buffer), then each row's running sum and the texels into `out`.  The LCD filter
// of every glyph, from `src` into `dst`.  Bit for bit what launch_rasterize_lines and launch_lcd_filter make of each glyph.
void launch_coverage_batch(hipStream_t s, const float4* lines, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, float* acc, uint32_t* out);
void launch_lcd_filter_batch(hipStream_t s, const msdf::BatchGlyph* glyphs, const uint32_t* tile_glyph, int n_tiles, const uint32_t* src, uint32_t* dst);
// fdh_put_image_sdf (include_glyphs/figdraw_hip_image_sdf.h; k_image_sdf.hip): byte `channel` of the sw x sh RGBA8 texels at `src`, `src_pitch`
// texels from row to row, is a coverage image; `out` takes its distance field of range `range` (1 .. 64), (sw + 2 pad) x (sh + 2 pad)
// texels, rows packed, the encoded distance in all four bytes
void launch_image_sdf_generate(hipStream_t s, const uint32_t* src, int sw, int sh, int src_pitch, int channel, int pad, int range, uint32_t* out);
// fdh_put_image_device and fdh_update_image_device (include_glyphs/figdraw_hip_device_image.h; k_image_import.hip; the parameter blocks:
// fdh_image_import.h): a source in device memory becomes levels 0 .. 5 of its atlas entry, a workgroup per 32 x 32 tile of the image, its
// level-5 image (a texel per tile) and, for a small image, its ink boxes; the tail makes the levels behind level P.l0 of that image
namespace image_import { struct Params; struct TailParams; }
void launch_image_import(hipStream_t s, const image_import::Params& P);
void launch_image_import_tail(hipStream_t s, const image_import::TailParams& P);
// fdh_put_images_device and fdh_update_images_device (include_glyphs/figdraw_hip_device_images.h): the same for the tiles of all images of one
// format of a batch -- a word per tile naming its image and its place in it, a record per image, the owner bits of the deep levels
// (fdh_image_batch.h) --, and the tails of all images that have one
namespace image_import { struct BatchImage; struct BatchAtlas; }
void launch_image_import_batch(hipStream_t s, uint32_t format, const image_import::BatchImage* images, const uint32_t* tiles, int n_tiles, const image_import::BatchAtlas& A,
                               uint32_t* scratch, int32_t* ink_blocks, const uint32_t* owner);
void launch_image_import_tail_batch(hipStream_t s, const image_import::BatchImage* images, const uint32_t* tails, int n_tails, const image_import::BatchAtlas& A, const uint32_t* scratch,
                                    const uint32_t* owner);
// fdh_put_video_frame and fdh_update_video_frame (include_glyphs/figdraw_hip_video_frame.h; k_video_import.hip; the parameter block:
// fdh_video_import.h): launch_image_import for an NV12, P010 or BGRA8 frame; launch_image_import_tail finishes its chain too
namespace video_import { struct Params; }
void launch_video_import(hipStream_t s, const video_import::Params& P);
// fdh_put_video_frames and fdh_update_video_frames (include_glyphs/figdraw_hip_video_frames.h): the same for the tiles of all frames of one
// group of a batch (video_import::batch_group) -- a word per tile naming its frame and its place in it, a record per frame, the owner bits
// of the deep levels (fdh_video_batch.h); launch_image_import_tail_batch finishes the chains
namespace video_import { struct BatchFrame; }
void launch_video_import_batch(hipStream_t s, int group, const video_import::BatchFrame* frames, const uint32_t* tiles, int n_tiles, const image_import::BatchAtlas& A, uint32_t* scratch,
                               int32_t* ink_blocks, const uint32_t* owner);
// fdh_read_video_frame (include_video/figdraw_hip_video_out.h; k_video_export.hip; the parameter block: fdh_video_export.h): the P.w x P.h
// texels at P.src out as NV12, P010 or BGRA8 planes, a workgroup per 128 x 16 tile of them
namespace video_export { struct Params; }
void launch_video_export(hipStream_t s, const video_export::Params& P);
// fdh_put_video_planes, fdh_update_video_planes and fdh_read_video_planes (include_video/figdraw_hip_video_planar.h; k_video_planar_import.hip,
// k_video_planar_export.hip; the parameter blocks: fdh_video_planar.h): the two launches above for three-plane frames, I420, I010, I444
// and I410 -- a workgroup of 128 per 32 x 32 tile on the way in (launch_image_import_tail finishes its chain too), a workgroup of 256 per
// 256 x 16 tile on the way out
namespace video_planar { struct InParams; struct OutParams; }
void launch_video_planar_import(hipStream_t s, const video_planar::InParams& P);
void launch_video_planar_export(hipStream_t s, const video_planar::OutParams& P);
// fdh_put_video_422, fdh_update_video_422 and fdh_read_video_422 (include_video/figdraw_hip_video_422.h; k_video_422_import.hip,
// k_video_422_export.hip; the parameter blocks: fdh_video_422.h): the same two launches for 4:2:2 frames, I422 and I210 in three planes
// and YUY2 and UYVY in one -- a workgroup of 128 per 32 x 32 tile on the way in (launch_image_import_tail finishes its chain too), a
// workgroup of 256 per 256 x 8 tile on the way out
namespace video_422 { struct InParams; struct OutParams; }
void launch_video_422_import(hipStream_t s, const video_422::InParams& P);
void launch_video_422_export(hipStream_t s, const video_422::OutParams& P);
// fdh_put_video_alpha, fdh_update_video_alpha and fdh_read_video_alpha (include_video/figdraw_hip_video_alpha.h; k_video_alpha_import.hip,
// k_video_alpha_export.hip; the parameter blocks: fdh_video_alpha.h): the same two launches for frames with an alpha plane, A420, A444,
// A410 and UYVA -- a workgroup of 128 per 32 x 32 tile on the way in (launch_image_import_tail finishes its chain too), a workgroup of
// 256 per 256 x 16 tile (A420) or 256 x 8 tile (the others) on the way out
namespace video_alpha { struct InParams; struct OutParams; }
void launch_video_alpha_import(hipStream_t s, const video_alpha::InParams& P);
void launch_video_alpha_export(hipStream_t s, const video_alpha::OutParams& P);
// fdh_compact_atlas (include_glyphs/figdraw_hip_atlas.h; k_atlas_move.hip): the rectangles of `records` (fdh_atlas_move.h) from the levels of one
// atlas into those of another, or from / into the dense buffers of V; `tile_record`: the record of each of the n_tiles tiles, the 1-D grid;
// `owner`: one bit per texel of the records that share texels with a later rectangle
namespace move { struct Views; struct Record; }
void launch_atlas_move(hipStream_t s, const move::Views& V, const move::Record* records, const uint32_t* tile_record, int n_tiles, const uint32_t* owner);
// The frame upload (k_upload_frame): a table of runs, each `bytes` of pinned host memory (its device view) going to byte offset
// dst_off of the frame block.  kind 0: 16-byte units; 1: BinRecs -- copied in 8-byte units, and the lane that carries a record's
// pixel bounds also writes the draw's 4-byte bin box; 2: DrawRecs -- 16-byte units, and the `ext` of every F_GENERAL record gets
// ext_add (extension indices are relative to the recording thread's array).  The table travels in the kernel arguments (4 KB at most).
constexpr int kMaxUploadRuns = 96;
struct UploadRun { const void* src; uint32_t dst_off, bytes, ext_add, kind; };
struct UploadTable {
  uint32_t n_runs, copy_units, n_draws, binbox_shift;
  uint32_t bins_off, box_off, _pad0, _pad1;     // byte offsets of the BinRec / bin box arrays in the block
  uint32_t unit_first[kMaxUploadRuns];           // the first 1-KB unit of run r (ascending)
  UploadRun run[kMaxUploadRuns];
};
static_assert(sizeof(UploadTable) <= 4096, "the table must fit the kernel-argument segment");
void launch_upload_frame(hipStream_t s, void* dst, const UploadTable& T);

}  // namespace fdh
