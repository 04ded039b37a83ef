// k_composite.hip -- the fused tile compositor: atlas.frag's main() (glsl/atlas.frag:252-405), the fixed-function blend and the RGBA8
// re-quantisation per draw (utils/glutils.nim:150-154), clip and rect masks, as ONE launch per phase of a frame.
//
//   k_composite_tiles  one single-wave workgroup per 32x8-pixel strip (four 8x8 tiles side by side, four pixels per lane)
//                      walks the bin's list in painter's order keeping RGBA in registers, re-quantising to RGBA8 after every
//                      draw like the GL framebuffer does, and stores the strip once.  Five builds picked per phase: <4> SDF draws
//                      only, <0> + clip masks, <2> + the 4-wide atlas path, <8> + rotated SDF quads, <3> + everything (one pixel slot at a time)
//   k_composite_deep   the full-frame launch of a frame with deep lists (round 6): workgroups of four waves, the strips of the deepest
//                      bins shaded by three waves and blended by a fourth
//   blocks::k_composite_tiles  the full-frame launch of <4> / <4 | 32> while other contexts render: one wave per 32 x 32 block (four strips,
//                      one after the other) in the bins with short lists
//
// Two translation units from this one file (csrc/Makefile).  FDH_TU 0 (this file as it is): the builds <3>, <19> and <8> and the
// dispatch (composite_build).  FDH_TU 1 (k_composite_uniform.hip): <0>, <2>, <4>, k_composite_deep and their launchers only, compiled with
// -structurizecfg-skip-uniform-regions.  hipcc structurizes EVERY region of a kernel's control flow, uniform branches
// included; in the draw loop that turns each wave-uniform branch into a predicate in an SGPR pair (s_cselect_b64 / s_and_b64
// / s_cbranch_vccnz where one s_cbranch_scc would do) and keeps the texels that merge at the loop latch out of the
// registers they came from (eight v_mov_b64 per draw).  With the switch, a region whose branches are all wave-uniform is
// left as the branches it is: phase 0 of the bench frame 38 -> 34 us, and with the registers that freed, six waves per SIMD.
// The switch is NOT safe for code that nests uniform branches inside divergent ones: with it the slot path <3> and the blur
// passes come out wrong (measured: 23 of the 57 GPU parity tests fail), so it stays confined to kernels whose draw loop
// nest holds no divergent branch at all -- tools/lint_isa.py checks exactly that on the built code object after every
// build, and the note at shadow_profile() says how the source keeps it so.  Instrumented builds (FDH_STATS, FDH_TIMING:
// device-side counters) are single-unit builds (`make variant SINGLE=1`).
#include "fdh_device.h"
#include "fdh_shade.h"
#include "fdh_damage.h"

#ifndef FDH_TU
#define FDH_TU 0
#endif

namespace fdh {

// Longest-processing-time-first order for the compositor: bins sorted by list length, descending (counting sort on
// min(count, 255); the order among equal keys is whatever the LDS atomics give -- bins are independent, only the
// schedule changes).  A strip's cost is roughly its list length, and a launch ends when its last wave does: started in
// frame order, a 60-entry strip picked up near the end ran on alone for a fifth of the kernel (58 -> 48 us).  The sort is
// done by ONE wavefront with 256 words of LDS, from inside k_composite_tiles (see there)
// (round 3: ONE CLASS of bins per wave -- the bins with index congruent to `cls` mod 8, written to the positions congruent to
// cls mod 8 of `order`.  The compositor hands position p to XCD p % 8 and k_bin_draws builds bin b's list on XCD b % 8: with the
// order sorted per class, a bin's list, its count and -- next frame -- its order entry are read on the XCD whose L2 they were
// written in, instead of being pulled across XCDs at the very start of every strip's life.)
// (round 6: the wave also leaves, in pinned host memory, how many bins of its class hold at least `deep_min` draws -- the exclusive
// prefix of that bucket of the descending histogram.  The host sizes the NEXT launches' deep-strip part from it: k_composite_deep.)
__device__ __forceinline__ void order_bins_wave(const uint32_t* __restrict__ counts, int* __restrict__ order, int nx, int nb, uint32_t* offs, int lane, int cls,
                                                int deep_min = 0, uint32_t* __restrict__ deep_out = nullptr, int block_max = 0) {
#pragma unroll
  for (int k = 0; k < 4; k++) offs[lane + 64 * k] = 0;
  __builtin_amdgcn_wave_barrier();
  constexpr int kU = 8;
  const int nc = (nb - cls + 7) >> 3;  // bins of this class: cls, cls + 8, ...
  for (int i0 = lane; i0 < nc; i0 += 64 * kU) {
    uint32_t c[kU];
#pragma unroll
    for (int k = 0; k < kU; k++) c[k] = i0 + 64 * k < nc ? counts[cls + 8 * (i0 + 64 * k)] : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kU; k++) if (c[k] != 0xffffffffu) atomicAdd(&offs[255u - min(c[k], 255u)], 1u);
  }
  __builtin_amdgcn_wave_barrier();
  {
    const uint32_t a = offs[4 * lane], b = offs[4 * lane + 1], c2 = offs[4 * lane + 2], d = offs[4 * lane + 3];
    uint32_t incl = a + b + c2 + d;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
      const uint32_t up = __shfl_up(incl, sh, 64);
      if (lane >= sh) incl += up;
    }
    const uint32_t base = incl - (a + b + c2 + d);
    __builtin_amdgcn_wave_barrier();
    offs[4 * lane] = base; offs[4 * lane + 1] = base + a; offs[4 * lane + 2] = base + a + b; offs[4 * lane + 3] = base + a + b + c2;
  }
  __builtin_amdgcn_wave_barrier();
  // bucket k holds the bins with min(count, 255) = 255 - k: counts >= m are buckets 0 .. 255 - m, the start of bucket 256 - m
  if (deep_out != nullptr && lane == 0) {
    const int m = min(max(deep_min, 1), 255);
    __hip_atomic_store(deep_out + cls, offs[256 - m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // (block waves: the bins of the class with MORE than block_max draws -- the positions of the order that keep one wave per strip)
    if (block_max > 0) __hip_atomic_store(deep_out + 8 + cls, offs[255 - min(block_max, 254)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __builtin_amdgcn_wave_barrier();
  for (int i0 = lane; i0 < nc; i0 += 64 * kU) {
    uint32_t c[kU];
#pragma unroll
    for (int k = 0; k < kU; k++) c[k] = i0 + 64 * k < nc ? counts[cls + 8 * (i0 + 64 * k)] : 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kU; k++)
      if (c[k] != 0xffffffffu) {  // stored as (row << 16 | column) of the launch's bin grid: the reader is spared a division
        const int i = cls + 8 * (i0 + 64 * k), row = i / nx;
        order[8 * (int)atomicAdd(&offs[255u - min(c[k], 255u)], 1u) + cls] = (row << 16) | (i - row * nx);
      }
  }
}

// ---- branch-free shape distance: no per-lane exec juggling (divergent control flow is paid in
// s_and_saveexec/s_or sequences on the CU's single scalar unit).  The two-sqrt ellipse evaluation is skipped with
// ONE wave-uniform branch when no lane of the wave sits in an elliptical corner region.
struct Corner { float rx, ry; bool same; };
__device__ __forceinline__ Corner pick_corner(bool ellip, float px, float py, float bx, float by, float r0, float r1, float r2, float r3) {
  const float sel = (px > 0.0f) ? ((py > 0.0f) ? r0 : r1) : ((py > 0.0f) ? r2 : r3);
  Corner c;
  if (!ellip) { c.rx = sel; c.ry = sel; c.same = true; return c; }  // wave-uniform
  // decodeEllipticalCornerRadii atlas.frag:88-94; negative = circular corner of radius -v-1 (:98-100)
  const float pv = __builtin_floorf(sel + 0.5f);
  const float hi = __builtin_floorf(pv * (1.0f / 4096.0f));
  float rx = (pv - 4096.0f * hi) * bx * (1.0f / 4095.0f);
  float ry = hi * by * (1.0f / 4095.0f);
  const bool circle = sel < 0.0f;
  const float rc = -sel - 1.0f;
  rx = circle ? rc : rx;
  ry = circle ? rc : ry;
  const bool zero = rx <= 0.0f || ry <= 0.0f;  // :102-105 -> plain box, i.e. the rounded-box formula with r = 0
  c.rx = zero ? 0.0f : rx;
  c.ry = zero ? 0.0f : ry;
  c.same = c.rx == c.ry;
  return c;
}
__device__ __forceinline__ float sd_ellipse_nb(float px, float py, float rx, float ry) {  // atlas.frag:71-79 without branches
  const float sx = __builtin_fmaxf(rx, 0.000001f), sy = __builtin_fmaxf(ry, 0.000001f);
  const float isx = frcp(sx), isy = frcp(sy);
  const float ax = px * isx, ay = py * isy;
  const float k0 = fsqrt(ax * ax + ay * ay);
  const float bx = ax * isx, by = ay * isy;
  const float k1 = fsqrt(bx * bx + by * by);
  const float d = k0 * (k0 - 1.0f) * frcp(__builtin_fmaxf(k1, 0.000001f));
  const float inner = -__builtin_fminf(sx, sy);  // (both arms are plain values: see the note on selects at shadow_profile)
  return k0 <= 0.000001f ? inner : d;
}
// distance of N pixels at once (sdRoundedBox :51-69 / sdEllipticalRoundedBox :96-115): of one row (kPerY = false: they share
// their local y, *pyv) or each with a local y of its own (rotated quads: pyv[k])
template <int N, bool kPerY>
__device__ __forceinline__ void shape_distNy(bool ellip, const float* px, const float* pyv, float bx, float by, float r0, float r1, float r2,
                                             float r3, float* out) {
  Corner c[N];
  float qx[N], qy[N];
  bool need = false, diag = false;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const float py = pyv[kPerY ? k : 0];
    c[k] = pick_corner(ellip, px[k], py, bx, by, r0, r1, r2, r3);
    qx[k] = __builtin_fabsf(px[k]) - bx + c[k].rx;
    qy[k] = __builtin_fabsf(py) - by + c[k].ry;
    const bool corner = qx[k] > 0.0f && qy[k] > 0.0f;
    diag = diag || corner;
    need = need || (!c[k].same && corner);
  }
  // length(max(q, 0)) only needs the (quarter-rate) sqrt where BOTH components are positive, i.e. in the corner
  // arcs; elsewhere it is max(qx, qy, 0).  One wave-uniform branch skips the sqrt for every strip without an arc.
  const bool any_diag = __any(diag);
  // (min(max(q.x, q.y), 0) + length(max(q, 0)) = (both components positive ? |q| : max(q.x, q.y)), exactly: see dist4 in
  // k_composite_tiles)
#pragma unroll
  for (int k = 0; k < N; k++) {
    float m = __builtin_fmaxf(qx[k], qy[k]);
    if (any_diag) {  // wave-uniform
      const float e = fsqrt(qx[k] * qx[k] + qy[k] * qy[k]);
      m = (qx[k] > 0.0f && qy[k] > 0.0f) ? e : m;
    }
    out[k] = m - c[k].rx;
  }
  if (!ellip) return;  // wave-uniform
  const bool any_ellipse = __any(need);
#pragma unroll
  for (int k = 0; k < N; k++) {
    const bool corner = qx[k] > 0.0f && qy[k] > 0.0f;
    float de = __builtin_fmaxf(qx[k] - c[k].rx, qy[k] - c[k].ry);
    if (any_ellipse) {  // wave-uniform
      const float e = sd_ellipse_nb(qx[k], qy[k], c[k].rx, c[k].ry);
      de = corner ? e : de;
    }
    out[k] = c[k].same ? out[k] : de;
  }
}
template <int N>
__device__ __forceinline__ void shape_distN(bool ellip, const float* px, float py, float bx, float by, float r0, float r1, float r2,
                                            float r3, float* out) {
  shape_distNy<N, false>(ellip, px, &py, bx, by, r0, r1, r2, r3, out);
}

// One wavefront = one 32x8 pixel tile: lane l owns the 4 horizontally adjacent pixels x = tx0 + 4*(l&7) .. +3 of
// row ty0 + (l>>3) -- i.e. four side-by-side 8x8 sub-tiles shaded in lock-step, so every record fetch, mode
// dispatch and loop step is paid once per 256 pixels, loads/stores of the surface are 16 B per lane and a wave
// reads or writes 8 full 128-byte lines.  A workgroup is ONE wavefront; the sixteen strips of a 64x64 bin are sixteen
// consecutive workgroups of an XCD.
//
// Axis-aligned SDF draws (fills, strokes, shadows, clip pushes, blur composites -- all but a handful of calls in
// real scenes) take the 4-wide straight-line path.  Everything else goes through shade_one() one pixel slot at a
// time; the per-lane state arrays are rotated between slots so they are only ever indexed statically.
// The builds without the one-pixel-slot path (phases made only of axis-aligned SDF draws, clips, axis-aligned atlas quads:
// no rotated quads, no bezier strokes, no rect-mask setup) need no scratch: 80 - 96 VGPRs, five or six waves per SIMD.
constexpr int kFastWaves = 5;
constexpr int kAtlasWaves = 5;  // waves per SIMD of the atlas build <2>
constexpr int kSlowWaves = 4;  // waves per SIMD of the build with every path <3>
// (<19> = <3> at three: a phase with atlas quads off the 4-wide path -- rotated glyph rows, minified images -- holds sixteen to thirty-two
// texels per lane and spills 47 registers at 128; config 11 243 -> 223 us at 168 registers, while the curves of config 10, all arithmetic,
// lose 7 % of their waves' overlap there (136 -> 146 us): the phase's content picks the form, fdh_record.cpp's has_slow_atlas)
constexpr int kSlowAtlasWaves = 3;
constexpr int kRotWaves = 4;  // waves per SIMD of the rotated-quad build <8>
constexpr int kUniformWaves = 6;  // waves per SIMD of the no-clip build <4>: 80 VGPRs, no spills
// the strip's texel window in LDS (builds with the atlas path): up to kWinCols x kWinRows texels, rows kWinStride dwords apart
// (a multiple of four, for the 16-byte stores, that is not a multiple of 32: rows start in different banks)
constexpr int kWinCols = 64, kWinRows = 12, kWinStride = 68;
// kPaths: bit 3 = the 4-wide path for rotated / skewed SDF quads (F_EDGE32) on top of the axis-aligned SDF paths, with clip masks:
// build <8>, for phases whose only draws off the fast paths are such quads (a rotated panel does not drag the slot path in);
// bit 0 = the one-pixel-slot path (rotated / skewed quads, bezier strokes, rect-mask setup, minified images),
// bit 1 = the 4-wide atlas path (axis-aligned glyphs, images at >= 1:1, MSDF).  0: SDF draws, clips and rect masks only.
// bit 5 = the surface is known opaque (CompositeParams::opaque): <4 | 32>, the no-clip build without the texels' alpha lane (F4o,
// fdh_device.h) -- same pixels as <4>, two of eight blend instructions per pixel and draw fewer.  Launches that walk lists only: a direct
// launch (its opaque form came out with two spilled vector registers where <4, ., direct> has none, and a frame of a handful of draws is
// latency, not arithmetic), a deep launch and a tracked frame's launches keep the generic <4>.
// kFull: the launch that starts a frame -- every bin of the grid, from the clear colour (nothing is loaded), bins taken longest
// list first, with the sort for the next frame riding along.  A symbol of its own, so that the dominant launch of a frame is a
// row of its own in a rocprofv3 kernel summary (the later phases' launches cover a blur node's footprint and take microseconds).
// ---- Deep strips (round 6).  A wave walks its strip's list one draw after the other, and alone on a SIMD it gets through a draw's ~200
// dependent instructions no faster than with five neighbours: at 1920 x 1080 the bench tree's lists are four times as deep as at 4K, and
// the full-frame launch was the serial chain of its longest strips -- the 128 strips of the eight longest bins, shaded with NOTHING else on
// the chip, take the launch's whole 29 us (profiles/r06_1080p_critical_path.txt).  What is serial in a strip is only the BLEND -- a draw's
// source term (coverage from the distance field, colour from the fill) depends on nothing before it.  So the strips of the frame's deepest
// bins get a workgroup of four waves (k_composite_deep): waves 1..3 (kRole 2, "shaders") each take every third draw that needs per-pixel
// work, evaluate its source term with the code below and put it into a ring of slots in LDS; wave 0 (kRole 1, the "blender") walks the same
// list, blends the one-colour core strips itself and every other draw's source term out of the ring, in list order.  Same operations on the
// same values as one wave would do (the blender's arithmetic is the tail of edge_blend / shade, moved): bit-identical frames.
// Slot payload per lane: packed edge paths 4 floats (the four source alphas; the draw's colour rides in the slot's header), the generic path
// 16 (r, g, b, masked alpha of the four pixels).
constexpr int kDeepSlots = 6;                               // ring depth: source terms a strip's shaders may be ahead of its blender
constexpr int kDeepSlotFloats = 16 * 64;                    // 4 KB of payload per slot: [float index 0..15][lane]
constexpr int kDeepHdr = 8;                                 // dwords of header per slot: tag, colour words / uniform terms
[[maybe_unused]] constexpr int kDeepLdsDwords = kDeepSlots * (kDeepSlotFloats + kDeepHdr) + kDeepSlots + 2;  // + ready[] + consumed
constexpr uint32_t DT_NOP = 0, DT_PACKED = 1, DT_PACKED_BLACK = 2, DT_GENERIC = 3, DT_SELF17 = 4, DT_UNIFORM_PRE = 5;
struct DeepRing {
  float* data;         // [slot][16][64]
  uint32_t* hdr;       // [slot][kDeepHdr]
  uint32_t* ready;     // [slot]: rank + 1 of the source term the slot holds
  uint32_t* consumed;  // ranks the blender is done with
  __device__ __forceinline__ explicit DeepRing(uint32_t* lds)
      : data(reinterpret_cast<float*>(lds)), hdr(lds + kDeepSlots * kDeepSlotFloats), ready(lds + kDeepSlots * (kDeepSlotFloats + kDeepHdr)),
        consumed(lds + kDeepSlots * (kDeepSlotFloats + kDeepHdr) + kDeepSlots) {}
};
// (a wait that can never be satisfied must not hang the device: after ~2^20 polls a wave goes on -- wrong pixels, which the tests see)
__device__ __forceinline__ void deep_wait_ge(const uint32_t* p, const uint32_t want) {
  for (int spins = 0; spins < (1 << 20); spins++) {
    const uint32_t v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
    if ((int32_t)(v - want) >= 0) return;
    __builtin_amdgcn_s_sleep(1);
  }
}

// How many draws of its list a strip has to SHADE -- survivors of the strip test and of the occlusion cut that are not one-colour core strips
// (those are a uniform blend: cheap) --, counted the way the draw loop walks the list.  A strip of a deep bin goes to k_composite_deep when
// this reaches P.deep_strip_min, and to its usual wave otherwise: both kernels ask this function, so they agree.
__device__ __forceinline__ uint32_t strip_shade_count(const CompositeParams& P, const int bin, const int sbit, const int lane) {
  const uint32_t cnt = P.counts[bin];
  const uint2* __restrict__ list = P.lists + (size_t)bin * P.stride;
  uint32_t n = 0;
  for (uint32_t base = 0; base < cnt; base += 64) {
    const uint32_t i = base + lane;
    const uint2 e = list[min(i, cnt - 1u)];
    const uint32_t ey = i < cnt ? e.y : 0u;
    const uint32_t st = (ey >> sbit) & 0x10001u;
    unsigned long long m = __ballot(st != 0u);
    const unsigned long long m_opaque = __ballot(st == 0x10001u && (e.x & LE_OPAQUE) != 0u);
    if (m_opaque != 0) m &= ~((1ull << (63 - __builtin_clzll(m_opaque))) - 1ull);
    m &= ~__ballot(st == 0x10001u && (int32_t)e.x < 0);
    n += (uint32_t)__builtin_popcountll(m);
  }
  return n;
}

template <int kPaths, bool kFull, int kRole, bool kDirect = false, bool kInterior = false>
__device__ __forceinline__ void composite_strip(const CompositeParams& P, const DrawRec* __restrict__ draws, const QuadExt* __restrict__ exts,
                                                uint32_t* composite_lds, const int bin, const int sidx, const int sbit, const int tx0, const int ty0,
                                                const int lane, const int shader_id, const uint32_t cnt_in = 0);

template <int kPaths, bool kFull, bool kDirect = false>
__global__ __launch_bounds__(64, (kPaths & 16) ? kSlowAtlasWaves : (kPaths & 1) ? kSlowWaves : (kPaths & ~32) == 4 ? kUniformWaves : (kPaths & 2) ? kAtlasWaves : (kPaths & 8) ? kRotWaves : kFastWaves) void k_composite_tiles(
    // the sixteen dwords a wave needs before anything else, as leading scalar arguments: with kernel-argument preloading
    // (-amdgpu-kernarg-preload-count, csrc/Makefile) they arrive in SGPRs with the wave instead of through a first s_load
    const int* __restrict__ a_order, int* __restrict__ a_order_next, const uint32_t* __restrict__ a_counts, const uint2* __restrict__ a_lists,
    int a_bin_x0, int a_bin_y0, int a_bin_nx, int a_bin_ny, int a_bins_x, int a_stride, int a_row_lo, int a_row_hi,
    const DrawRec* __restrict__ draws, const QuadExt* __restrict__ exts, const CompositeParams P_in) {
  // (a copy, so that the preloaded arguments can take their fields' places -- and the atlas read through the ORIGINAL: a mip level is picked by
  // a run-time index, and an indexed member of a struct the kernel writes to keeps the WHOLE struct in scratch memory: the <3> build read
  // every field of its 312-byte copy from there, tools/kernel_regs.py)
  CompositeParams P = P_in;
  [[maybe_unused]] const AtlasView& atlas_view = P_in.atlas;
  P.order = kFull ? a_order : nullptr; P.order_next = kFull ? a_order_next : nullptr; P.counts = a_counts; P.lists = a_lists;
  if (kFull) P.load_fb = 0;
  P.bin_x0 = a_bin_x0; P.bin_y0 = a_bin_y0; P.bin_nx = a_bin_nx; P.bin_ny = a_bin_ny;
  P.bins_x = a_bins_x; P.stride = a_stride; P.row_lo = a_row_lo; P.row_hi = a_row_hi;
  // clip stack: 4 pixels' q8 mask values packed per lane and level.  Dynamic LDS: 4 KB when the phase has clip operations,
  // 1 KB (what the bin-ordering wavefront needs) when it has none -- a phase's waves then fit beside the 18-KB rings of
  // another frame's blur pass on the same CU (20 x 4 KB + 8 x 18 KB do not)
  extern __shared__ uint32_t composite_lds[];
  uint32_t (*mask_stack)[kMaskDepth][64] = reinterpret_cast<uint32_t (*)[kMaskDepth][64]>(composite_lds);
  // XCD-aware mapping: the dispatcher places workgroup b on XCD b % 8.  XCD x takes the bins x, x+8, x+16, ... of this
  // launch (row-major), all 16 strips of a bin back to back: a bin's draw list and records stay in ONE L2, and every
  // XCD gets an even sample of the frame -- contiguous bands per XCD left the XCDs holding the busy rows 3x the work
  // of the ones holding the emptier top and bottom of the frame.
  constexpr int kStripsPerBin = kWgsPerBin * kWavesPerWg;  // 16
  // (a workgroup is ONE wavefront: nothing is shared between strips, and the dispatcher refills wave slots one at a time)
  // (with a sort riding along, the first eight workgroups are its -- one per XCD, each sorts the bins of its class --, dispatched
  // first so they are done long before the launch ends; the numbering of the rest shifts by eight and keeps its XCD phase)
  const int blk = P.order_next ? (int)blockIdx.x - 8 : (int)blockIdx.x;
  const int q = blk >> 3, xcd = blk & 7;
  if (blk < 0) {
    // One extra wavefront per full-frame launch sorts THIS frame's bin counts for the NEXT frame's launch (any
    // permutation is a correct schedule, and list lengths barely change from frame to frame).  As a kernel of its own the
    // sort was a ~6 us serial step of every frame; here it runs beside 32 000 compositing waves.
    order_bins_wave(P.counts, P.order_next, P.bin_nx, P.bin_nx * P.bin_ny, &mask_stack[0][0][0], threadIdx.x, (int)blockIdx.x, (kPaths & ~32) == 4 ? P.deep_min : 0, (kPaths & ~32) == 4 ? P.deep_out : nullptr, (kPaths & ~32) == 4 ? P.block_max : 0);
    return;
  }
  int bin_local = xcd + 8 * (q / kStripsPerBin);
  const int sidx = q % kStripsPerBin;
  if (bin_local >= P.bin_nx * P.bin_ny) return;
  const int j = sidx >> 2, wave = sidx & 3, lane = threadIdx.x & 63;
  const int sbit = j * 4 + wave;  // this strip's bit in the list entries' strip masks
  int bly, blx;
  if (P.order) {  // longest lists first (order_bins_wave): entries are row << 16 | column
    const int rc = P.order[bin_local];
    bly = rc >> 16; blx = rc & 0xffff;
  } else {
    bly = bin_local / P.bin_nx; blx = bin_local - bly * P.bin_nx;
  }
  const int bin_x = P.bin_x0 + blx, bin_y = P.bin_y0 + bly;
  const int bin = bin_y * P.bins_x + bin_x;
  const int tx0 = bin_x * kBin + (j & 1) * kWgW;
  const int ty0 = bin_y * kBin + (j >> 1) * kWgH + wave * kTileH;
  // (four plain scalar compare-and-branch pairs: written with ||, each pair became two s_cselect_b64 masks, an s_and_b64 and a vcc branch)
  // (the empty asm statements keep the compiler from folding the four exits back into that form)
  if (tx0 >= P.W) return;
  asm volatile("");
  if (ty0 >= P.H) return;
  asm volatile("");
  if (ty0 + kTileH <= P.row_lo) return;
  asm volatile("");
  if (ty0 >= P.row_hi) return;
  // The strip's shading, k_composite_strip.inc: as a CALL in the uniform-regions unit and as TEXT in the other.  Same source either way, but
  // the register allocator lands elsewhere: called, the bench frame's <4, true> has no spilled scalar register (as text: nine), and as text the
  // <3> build keeps round 5's size and scratch (called: 9 KB more code than the instruction cache likes, config 10 19 % slower) --
  // same-box A/B against round 5's library in profiles/r06_ab_r05g.txt.
#if FDH_TU == 1
  composite_strip<kPaths, kFull, 0, kDirect>(P, draws, exts, composite_lds, bin, sidx, sbit, tx0, ty0, lane, 0);
#else
  constexpr int kRole = 0;
  constexpr int shader_id = 0;
  constexpr bool kInterior = false;
  constexpr uint32_t cnt_in = 0;
  {  // (a scope of its own: the body names some of what the mapping above has named)
#include "k_composite_strip.inc"
  }
#endif
}

// ---- Block waves.  The full-frame launch of the no-clip builds for a frame ALL of whose strips are whole (composite_build: W a multiple of
// 32, H of 8, pitch of 4, no stripe) and whose order is at hand, laid out as k_composite_deep lays out its parts: the first P.block_k8
// positions of the order -- the bins with more than block_max draws, as the sorting waves of earlier frames counted them -- get sixteen
// one-wave workgroups each, one strip per wave as in k_composite_tiles above; every later position gets FOUR, and a wave shades the four
// vertically stacked strips 4 j .. 4 j + 3 of a 32 x 32 block one after the other: its dispatch and the dependent fetches of the order
// entry and the count are paid once per block, and the launch spends a sixth fewer wave cycles on the bench frame.  That pays where other
// contexts' launches take the wave slots, and costs where the frame has the GPU to itself -- a block's strips run in series at the END of
// the launch -- so Context::schedule asks for it only while other contexts are launching (profiles/block_waves.txt).  Both parts' sizes
// are multiples of 8: position p keeps XCD p % 8.  Any boundary gives the same pixels: the strip body is the same, with its prologue and
// epilogue in their interior form (no partial row or 16-byte group: no branch on the lane, which the loop around the body must not
// hold -- tools/lint_isa.py); a strip wholly below the frame is left out by the trip count.  The kernel keeps k_composite_tiles' name and
// arguments in a namespace of its own: a row of its own in a kernel summary, and the lint finds it by the name.
namespace blocks {
template <int kPaths, bool kFull, bool kDirect>
__global__ __launch_bounds__(64, kUniformWaves) void k_composite_tiles(
    const int* __restrict__ a_order, int* __restrict__ a_order_next, const uint32_t* __restrict__ a_counts, const uint2* __restrict__ a_lists,
    int a_bin_x0, int a_bin_y0, int a_bin_nx, int a_bin_ny, int a_bins_x, int a_stride, int a_row_lo, int a_row_hi,
    const DrawRec* __restrict__ draws, const QuadExt* __restrict__ exts, const CompositeParams P_in) {
  static_assert((kPaths & ~32) == 4 && kFull && !kDirect, "block waves: the no-clip builds' full-frame launch from the lists");
  CompositeParams P = P_in;
  P.order = a_order; P.order_next = a_order_next; P.counts = a_counts; P.lists = a_lists;
  P.load_fb = 0;
  P.bin_x0 = a_bin_x0; P.bin_y0 = a_bin_y0; P.bin_nx = a_bin_nx; P.bin_ny = a_bin_ny;
  P.bins_x = a_bins_x; P.stride = a_stride; P.row_lo = a_row_lo; P.row_hi = a_row_hi;
  extern __shared__ uint32_t composite_lds[];
  constexpr int kStripsPerBin = kWgsPerBin * kWavesPerWg;  // 16
  const int blk = (int)blockIdx.x - 8;  // (the launch has both order pointers: the first eight workgroups sort)
  if (blk < 0) {
    order_bins_wave(P.counts, P.order_next, P.bin_nx, P.bin_nx * P.bin_ny, composite_lds, threadIdx.x, (int)blockIdx.x, P.deep_min, P.deep_out, P.block_max);
    return;
  }
  const int q = blk >> 3, xcd = blk & 7;
  const int n_strip = P.block_k8 * kStripsPerBin;
  int bin_local, s0, ns;
  if (blk < n_strip) {
    bin_local = xcd + 8 * (q / kStripsPerBin); s0 = q % kStripsPerBin; ns = 1;
  } else {
    const int q2 = (blk - n_strip) >> 3;
    bin_local = P.block_k8 + xcd + 8 * (q2 >> 2); s0 = 4 * (q2 & 3); ns = 4;
  }
  if (bin_local >= P.bin_nx * P.bin_ny) return;
  const int rc = P.order[bin_local];
  const int bin_x = P.bin_x0 + (rc & 0xffff), bin_y = P.bin_y0 + (rc >> 16);
  const int bin = bin_y * P.bins_x + bin_x;
  const int jb = s0 >> 2;
  const int tx0 = bin_x * kBin + (jb & 1) * kWgW;
  const int ty0 = bin_y * kBin + (jb >> 1) * kWgH + (s0 & 3) * kTileH;
  if (tx0 >= P.W) return;
  ns = min(ns, (P.H - ty0) / kTileH);  // (H is a multiple of 8: a strip is inside the frame or below it)
  if (ns <= 0) return;
  const uint32_t cnt = P.counts[bin];
  for (int k = 0; k < ns; k++) {
    // (the lane index is derived again per strip, opaquely: what a strip computes from it is not kept in registers across the others' draw loops)
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    composite_strip<kPaths, true, 0, false, true>(P, draws, exts, composite_lds, bin, s0 + k, s0 + k, tx0, ty0 + k * kTileH, lane, 0, cnt);
  }
}
}  // namespace blocks

// The full-frame launch of a frame that HAS deep bins (P.deep_k8 > 0; k_composite_tiles<4, true> otherwise), workgroups of four waves:
//   workgroups 0..7: wave 0 of each sorts one class of this frame's bin counts for the next frame (order_bins_wave);
//   then 16 per bin of the first P.deep_k8 positions of `order`: one deep strip each -- if the strip has P.deep_strip_min draws to shade;
//   then 4 per bin of the frame: sixteen one-wave strips as k_composite_tiles shades them, four to a workgroup (a strip the deep part took
//   leaves its wave idle).
// One launch, so that the deep strips' shaders and blenders run BESIDE the other strips' waves: as a launch of their own in front they
// added their whole duration (sweeps in profiles/r06_deep_strips.txt).  Workgroup b runs on XCD b % 8; every part's size is a multiple of
// 8, so position p keeps XCD p % 8 in both parts, like the strips of k_composite_tiles.
template <int kUnit>  // (a template so that only the translation unit that launches it holds the symbol)
__global__ __launch_bounds__(256, kUniformWaves) void k_composite_deep(const DrawRec* __restrict__ draws, const QuadExt* __restrict__ exts, CompositeParams P) {
  extern __shared__ uint32_t composite_lds[];
  constexpr int kStripsPerBin = kWgsPerBin * kWavesPerWg;  // 16
  // (which wave of the workgroup this is, as a value the compiler KNOWS to be wave-uniform: taken from the thread index alone it counted as
  // divergent, and with it every branch on whose turn a shading unit is -- the whole draw loop ran under exec masks)
  const int lane = threadIdx.x & 63, wg_wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  int blk = (int)blockIdx.x - 8;
  if (blk < 0) {
    if (wg_wave == 0) order_bins_wave(P.counts, P.order_next, P.bin_nx, P.bin_nx * P.bin_ny, composite_lds, lane, (int)blockIdx.x, P.deep_min, P.deep_out, P.block_max);
    return;
  }
  const int n_deep = P.deep_k8 * kStripsPerBin;
  const bool deep = blk < n_deep;
  int bin_local, sidx;
  if (deep) {
    const int q = blk >> 3;
    bin_local = (blk & 7) + 8 * (q / kStripsPerBin);
    sidx = q % kStripsPerBin;
  } else {
    blk -= n_deep;
    const int q = blk >> 3;
    bin_local = (blk & 7) + 8 * (q >> 2);
    sidx = 4 * (q & 3) + wg_wave;
  }
  if (bin_local >= P.bin_nx * P.bin_ny) return;
  const int j = sidx >> 2, wave = sidx & 3;
  const int sbit = j * 4 + wave;
  const int rc = P.order[bin_local];
  const int bly = rc >> 16, blx = rc & 0xffff;
  const int bin_x = P.bin_x0 + blx, bin_y = P.bin_y0 + bly;
  const int bin = bin_y * P.bins_x + bin_x;
  const int tx0 = bin_x * kBin + (j & 1) * kWgW;
  const int ty0 = bin_y * kBin + (j >> 1) * kWgH + wave * kTileH;
  if (tx0 >= P.W || ty0 >= P.H || ty0 + kTileH <= P.row_lo || ty0 >= P.row_hi) return;
  const bool is_deep = bin_local < P.deep_k8 && strip_shade_count(P, bin, sbit, lane) >= (uint32_t)P.deep_strip_min;
  if (!deep) {  // one wave, one strip
    if (!is_deep) composite_strip<4, true, 0>(P, draws, exts, composite_lds, bin, sidx, sbit, tx0, ty0, lane, 0);
    return;
  }
  if (!is_deep) return;  // (the whole workgroup: one strip, one answer -- its usual wave shades it)
  if (threadIdx.x < kDeepSlots + 2) composite_lds[kDeepSlots * (kDeepSlotFloats + kDeepHdr) + threadIdx.x] = 0u;  // ready[], consumed
  __syncthreads();
  // (tried: s_setprio 3 / 2 for a deep strip's blender / shaders -- the launch takes the same time, profiles/r06_deep_strips.txt)
  if (wg_wave == 0) composite_strip<4, true, 1>(P, draws, exts, composite_lds, bin, sidx, sbit, tx0, ty0, lane, 0);
  else composite_strip<4, true, 2>(P, draws, exts, composite_lds, bin, sidx, sbit, tx0, ty0, lane, wg_wave - 1);
}

template <int kPaths, bool kFull, int kRole, bool kDirect, bool kInterior>
__device__ __forceinline__ void composite_strip(const CompositeParams& P, const DrawRec* __restrict__ draws, const QuadExt* __restrict__ exts,
                                                uint32_t* composite_lds, const int bin, const int sidx, const int sbit, const int tx0, const int ty0,
                                                const int lane, const int shader_id, const uint32_t cnt_in) {
  [[maybe_unused]] const AtlasView& atlas_view = P.atlas;
#include "k_composite_strip.inc"
}

// The compositor launch of a tracked frame (fdh_set_damage_tracking, fdh_damage.h): its waves take their strips from the compact list of
// damaged bins k_damage_resolve left (16 strips per listed bin) instead of from the launch's bin box or `order`; a listed bin outside this
// launch's box (a later phase's) is not this launch's.  The strip is shaded as k_composite_tiles shades it (composite_strip, the same build
// per kPaths); no sorting wave, no deep strips.  The grid is sized on the host before the count is known: one wave per strip of the frame,
// those beyond the list exiting at once.  (A fixed grid whose waves walk the listed strips was the first form: the loop around the strip
// puts the strip's divergent epilogue inside the draw loop nest, which the uniform-regions unit must not have -- tools/lint_isa.py --, and
// it spilled; profiles/damage_bench.txt.)
template <int kPaths, bool kFull>
__global__ __launch_bounds__(64, (kPaths & 16) ? kSlowAtlasWaves : (kPaths & 1) ? kSlowWaves : kPaths == 4 ? kUniformWaves : (kPaths & 2) ? kAtlasWaves : (kPaths & 8) ? kRotWaves : kFastWaves) void k_composite_damage(
    const int* __restrict__ dmg_list, const uint32_t* __restrict__ dmg_count, const DrawRec* __restrict__ draws, const QuadExt* __restrict__ exts,
    const CompositeParams P_in) {
  constexpr int kStripsPerBin = kWgsPerBin * kWavesPerWg;  // 16
  const int i = (int)blockIdx.x;
  if (i >= (int)dmg_count[0] * kStripsPerBin) return;
  CompositeParams P = P_in;
  P.order = nullptr; P.order_next = nullptr; P.deep_k8 = 0; P.deep_out = nullptr; P.direct = 0;
  if (kFull) P.load_fb = 0;
  extern __shared__ uint32_t composite_lds[];
  const int lane = threadIdx.x & 63;
  const int bin = dmg_list[i / kStripsPerBin];
  const int sidx = i % kStripsPerBin;
  const int bin_y = bin / P.bins_x, bin_x = bin - bin_y * P.bins_x;
  if (bin_x < P.bin_x0 || bin_x >= P.bin_x0 + P.bin_nx || bin_y < P.bin_y0 || bin_y >= P.bin_y0 + P.bin_ny) return;
  const int j = sidx >> 2, wave = sidx & 3;
  const int sbit = j * 4 + wave;
  const int tx0 = bin_x * kBin + (j & 1) * kWgW;
  const int ty0 = bin_y * kBin + (j >> 1) * kWgH + wave * kTileH;
  if (tx0 >= P.W) return;
  asm volatile("");
  if (ty0 >= P.H) return;
  asm volatile("");
  if (ty0 + kTileH <= P.row_lo) return;
  asm volatile("");
  if (ty0 >= P.row_hi) return;
  composite_strip<kPaths, kFull, 0>(P, draws, exts, composite_lds, bin, sidx, sbit, tx0, ty0, lane, 0);
}
// ---- The launches, all through FDH_LAUNCH (fdh_profile's events, when set, stamp them).  Which build a launch takes is composite_build's
// decision (FDH_TU 0); the uniform unit's builds and k_composite_deep are launched from that unit.
template <int kPaths, bool kFull, bool kDirect>
static void launch_tiles(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P) {
  FDH_LAUNCH((k_composite_tiles<kPaths, kFull, kDirect>), dim3(grid), dim3(64), b.lds, s, P.order, P.order_next, P.counts, P.lists, P.bin_x0, P.bin_y0,
             P.bin_nx, P.bin_ny, P.bins_x, P.stride, P.row_lo, P.row_hi, draws, exts, P);
}
template <int kPaths>  // (block waves: the full-frame launch of <4> / <4 | 32>, launch_composite_uniform)
[[maybe_unused]] static void launch_blocks(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P) {
  FDH_LAUNCH((blocks::k_composite_tiles<kPaths, true, false>), dim3(grid), dim3(64), b.lds, s, P.order, P.order_next, P.counts, P.lists, P.bin_x0, P.bin_y0,
             P.bin_nx, P.bin_ny, P.bins_x, P.stride, P.row_lo, P.row_hi, draws, exts, P);
}
template <int kPaths>  // (kFull: the launch that starts a frame)
static void launch_damage(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P,
                          const int* list, const uint32_t* count) {
  if (P.load_fb == 0) FDH_LAUNCH((k_composite_damage<kPaths, true>), dim3(grid), dim3(64), b.lds, s, list, count, draws, exts, P);
  else FDH_LAUNCH((k_composite_damage<kPaths, false>), dim3(grid), dim3(64), b.lds, s, list, count, draws, exts, P);
}
// build kPaths of P's launch: the launch that starts a frame (kFull) or a later phase's, from the lists or direct (the uniform unit's builds)
template <int kPaths>
static void launch_tiles_build(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P) {
  constexpr bool kHasDirect = kPaths == 0 || kPaths == 2 || kPaths == 4;
  const bool direct = kHasDirect && P.direct;
  if (P.load_fb == 0) direct ? launch_tiles<kPaths, true, kHasDirect>(s, b, grid, draws, exts, P) : launch_tiles<kPaths, true, false>(s, b, grid, draws, exts, P);
  else direct ? launch_tiles<kPaths, false, kHasDirect>(s, b, grid, draws, exts, P) : launch_tiles<kPaths, false, false>(s, b, grid, draws, exts, P);
}

// the uniform unit's builds <0|2|4>: its own launchers (and the single-unit build's)
void launch_composite_uniform(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P);
void launch_composite_damage_uniform(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P,
                                     const int* list, const uint32_t* count);
#if FDH_TU == 1 || !FDH_SPLIT_UNIFORM
void launch_composite_uniform(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P) {
  if (b.deep) {  // build <4>'s full-frame launch with deep bins: four-wave workgroups (a direct frame has no sort, so no deep strips)
    const int bins8 = (P.bin_nx * P.bin_ny + 7) / 8;
    FDH_LAUNCH((k_composite_deep<FDH_TU>), dim3(8 + P.deep_k8 * 16 + 8 * bins8 * kWgsPerBin), dim3(256), b.lds, s, draws, exts, P);
  } else if (b.block) {  // the full-frame launch of <4> / <4 | 32> with block waves (launch_composite has sized the grid for P.block_k8)
    if (b.paths == (4 | 32)) launch_blocks<4 | 32>(s, b, grid, draws, exts, P);
    else launch_blocks<4>(s, b, grid, draws, exts, P);
  } else if (b.paths == 2) launch_tiles_build<2>(s, b, grid, draws, exts, P);
  else if (b.paths == 0) launch_tiles_build<0>(s, b, grid, draws, exts, P);
  else if (b.paths == (4 | 32)) launch_tiles_build<4 | 32>(s, b, grid, draws, exts, P);
  else launch_tiles_build<4>(s, b, grid, draws, exts, P);
}
void launch_composite_damage_uniform(hipStream_t s, const CompositeBuild& b, int grid, const DrawRec* draws, const QuadExt* exts, const CompositeParams& P,
                                     const int* list, const uint32_t* count) {
  if (b.paths == 2) launch_damage<2>(s, b, grid, draws, exts, P, list, count);
  else if (b.paths == 0) launch_damage<0>(s, b, grid, draws, exts, P, list, count);
  else launch_damage<4>(s, b, grid, draws, exts, P, list, count);
}
#endif

#if FDH_TU == 0
CompositeBuild composite_build(CompositeParams& P) {
  switch (forced_kernel_paths()) {
    case 3: P.has_slow = 1; P.has_slow_atlas = 0; break;  // (<3> itself, also where the phase would take its 168-register form)
    case 19: P.has_slow = 1; P.has_slow_atlas = 1; break;
    case 8: P.has_rot = 1; break;
    case 2: P.has_atlas = 1; break;
    case 1: P.has_masks = 1; break;  // (the build with mask registers and the 4-KB stack, even where no clip is open)
  }
  CompositeBuild b;
  if (P.has_slow || (P.has_rot && P.has_atlas)) b.paths = P.has_slow_atlas ? 19 : 3;
  else if (P.has_rot) b.paths = 8;
  else b.paths = P.has_atlas ? 2 : P.has_masks ? 0 : 4;
  // deep strips (k_composite_deep): only beside the no-clip build's full-frame launch, and only with the order at hand
  const int bins8 = (P.bin_nx * P.bin_ny + 7) / 8;  // bins per XCD
  if (b.paths == 4 && P.load_fb == 0 && P.order && P.order_next) b.deep_k8 = std::min(P.deep_k8 & ~7, 8 * bins8);
  b.deep = b.deep_k8 > 0;
  // an opaque surface (Context::prepare decides per frame): the no-clip build without the alpha lane, where the launch walks lists with one
  // wave per strip.  (FDH_FORCE_KERNEL_PATHS has set the phase flags above: a forced build is not <4> and stays what was asked for.)
  if (b.paths == 4 && P.opaque && !b.deep && !P.direct) b.paths = 4 | 32;
  // block waves: the same launch -- one wave per strip, from the lists, with the order -- of a frame that has no partial strip
  if ((b.paths & ~32) == 4 && P.load_fb == 0 && P.order && P.order_next && !b.deep && !P.direct && P.block_k8 >= 0 && P.W % kTileW == 0 &&
      P.H % kTileH == 0 && P.pitch % 4 == 0 && P.row_lo <= 0 && P.row_hi >= P.H) {
    b.block = true;
    b.block_k8 = std::min(P.block_k8 & ~7, 8 * bins8);
  }
  // the clip stack (4 KB; 1 KB, what the bin-ordering wavefront needs, without clips) + the texel window of the atlas path; the deep launch: its ring
  b.lds = b.deep ? sizeof(uint32_t) * kDeepLdsDwords
                 : (P.has_masks ? sizeof(uint32_t) * kMaskDepth * 64 : sizeof(uint32_t) * 256) +
                       (P.has_atlas || P.has_slow ? sizeof(uint32_t) * kWinRows * kWinStride : 0);
  return b;
}
void launch_composite_damage(hipStream_t s, const DrawRec* draws, const QuadExt* exts, CompositeParams P, const int* list, const uint32_t* count,
                             int grid) {
  if (grid <= 0 || P.bin_nx <= 0 || P.bin_ny <= 0) return;
  P.opaque = 0;  // (k_composite_damage has the generic builds only: same pixels)
  const CompositeBuild b = composite_build(P);  // (a tracked frame's partial launches have no order: no deep strips)
  P.n_wg = grid;
  if (b.paths == 19) launch_damage<19>(s, b, grid, draws, exts, P, list, count);
  else if (b.paths == 3) launch_damage<3>(s, b, grid, draws, exts, P, list, count);
  else if (b.paths == 8) launch_damage<8>(s, b, grid, draws, exts, P, list, count);
  else launch_composite_damage_uniform(s, b, grid, draws, exts, P, list, count);
}
void launch_composite(hipStream_t s, const DrawRec* draws, const QuadExt* exts, CompositeParams P) {
  const int n = P.bin_nx * P.bin_ny * kWgsPerBin;
  if (n <= 0) return;
  const CompositeBuild b = composite_build(P);
  P.n_wg = n;
  P.deep_k8 = b.deep_k8;
  const int bins8 = (P.bin_nx * P.bin_ny + 7) / 8;  // bins per XCD
  int grid = 8 * bins8 * kWgsPerBin * kWavesPerWg + (P.order_next ? 8 : 0);  // 16 strips per bin, one wavefront each (+ the sorting ones)
  P.block_k8 = b.block ? b.block_k8 : -1;
  if (b.block) grid = 8 + b.block_k8 * kWgsPerBin * kWavesPerWg + (8 * bins8 - b.block_k8) * kWgsPerBin;  // (one wavefront per block behind the boundary)
  if (b.paths == 19) launch_tiles_build<19>(s, b, grid, draws, exts, P);
  else if (b.paths == 3) launch_tiles_build<3>(s, b, grid, draws, exts, P);
  else if (b.paths == 8) launch_tiles_build<8>(s, b, grid, draws, exts, P);
  else launch_composite_uniform(s, b, grid, draws, exts, P);
}
#endif  // FDH_TU
}  // namespace fdh
