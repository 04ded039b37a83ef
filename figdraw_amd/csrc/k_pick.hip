// k_pick.hip -- hit testing (include/figdraw_hip_pick.h): which draws of the last submitted frame reach a pixel, with the compositor's own
// per-pixel arithmetic (shade_one, fdh_shade.h) and its mask rules -- the clip stack stores q8(a * a) per level (a = the push's coverage
// times its parent level), the rect mask multiplies the source alpha by rect_mask_alpha().
//
//   k_pick<true>   region queries: one 256-thread workgroup per 16 x 16 tile of the rectangle, one thread per pixel; each keeps the last
//                  (= front-most) draw that hits its pixel
//   k_pick<false>  point queries: one workgroup per 16 x 16 tile that holds query points (sorted by tile on the host), one thread per
//                  point; each keeps a ring of its last max_hits hits
//
// Reads the frame block as the frame left it: DrawRec (the clipped pixel bounds bx0..by1, not the bin boxes -- a folded clear empties
// only record 0's bin box), QuadExt, the phase table and the atlas.  Works the same for direct, binned, damage-tracked and replayed frames:
// no bin list is read.  A workgroup first tests 64 records per wave step against its tile (one ballot per step; every clip and rect-mask
// record is kept whatever its bounds: a push that misses a pixel still opens a level whose value there is 0), then walks the survivors
// in painter's order, every thread its own pixel.  Vector stores only.
#include "fdh_device.h"
#include "fdh_shade.h"
#include "fdh_pick.h"

namespace fdh {

template <bool kRegion>
__global__ __launch_bounds__(kPickThreads) void k_pick(const PickParams P, const int spill_levels) {
  __shared__ unsigned long long keep[kPickWindow];  // survivor masks of the window's 64-record chunks
  __shared__ uint8_t stack[kPickDepth][kPickThreads];  // clip levels 0 .. kPickDepth - 1, q8 values
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = (int)blockIdx.x;
  int tx0, ty0, px, py, pt = -1;
  bool valid, in_rect = false;
  if (kRegion) {
    const int tyi = b / P.tiles_x, txi = b - tyi * P.tiles_x;
    tx0 = P.x0 + txi * kPickTile; ty0 = P.y0 + tyi * kPickTile;
    px = tx0 + (t % kPickTile); py = ty0 + t / kPickTile;
    in_rect = px < P.x0 + P.w && py < P.y0 + P.h;
  } else {
    const int2 o = P.tile_xy[b];
    tx0 = o.x; ty0 = o.y;
    const int first = P.tile_first[b], last = P.tile_first[b + 1];
    pt = first + t < last ? first + t : -1;
    const int2 q = pt >= 0 ? P.pts[pt] : make_int2(-1, -1);
    px = q.x; py = q.y;
  }
  valid = (kRegion ? in_rect : pt >= 0) && px >= 0 && py >= 0 && px < P.W && py < P.H;
  const size_t spill_at = (size_t)b * kPickThreads + (size_t)t, spill_stride = (size_t)gridDim.x * kPickThreads;
  auto put = [&](const int lvl, const uint32_t q) {
    if (lvl < kPickDepth) stack[lvl][t] = (uint8_t)q;
    else if (lvl - kPickDepth < spill_levels) P.spill[(size_t)(lvl - kPickDepth) * spill_stride + spill_at] = (uint8_t)q;
  };
  auto get = [&](const int lvl) -> uint32_t {
    if (lvl < kPickDepth) return stack[lvl][t];
    if (lvl - kPickDepth < spill_levels) return P.spill[(size_t)(lvl - kPickDepth) * spill_stride + spill_at];
    return 0u;
  };
  const F4 opaque = {255.0f, 255.0f, 255.0f, 255.0f};  // mode 17: the backdrop's own alpha does not count
  const float inv255 = 1.0f / 255.0f;
  const float thr = (float)P.threshold;
  int depth = 0;
  float mk = 1.0f, rm = 1.0f;  // open clip level, open rect mask
  int ph = 0;
  int next_pf = P.n_phases > 1 ? P.phase_first[1] : 0x7fffffff;
  int last_draw = -1, n_hits = 0;
  for (int w0 = 0; w0 < P.n_recs; w0 += kPickWindow * 64) {
    const int nch = min(kPickWindow, (P.n_recs - w0 + 63) >> 6);
    __syncthreads();  // (the previous window's walk is done with keep[])
    // (a wave takes four chunks per step, their loads issued before any of them is tested: one memory round trip per four chunks)
    constexpr int kU = 4, kWaves = kPickThreads / 64;
    for (int c0 = wave * kU; c0 < nch; c0 += kWaves * kU) {
      uint32_t om[kU], bxy[kU][2];
#pragma unroll
      for (int u = 0; u < kU; u++) {
        const int d = min(w0 + (c0 + u) * 64 + lane, P.n_recs - 1);
        const uint32_t* r = reinterpret_cast<const uint32_t*>(P.draws + d);
        om[u] = r[0];
        bxy[u][0] = r[offsetof(DrawRec, bx0) / 4];
        bxy[u][1] = r[offsetof(DrawRec, bx0) / 4 + 1];
      }
#pragma unroll
      for (int u = 0; u < kU; u++) {
        const int d = w0 + (c0 + u) * 64 + lane;
        const uint32_t op = (om[u] >> 12) & 15u, mode = om[u] & 255u;
        const bool shadow = mode >= 7u && mode <= 10u;
        const int bx0 = (int16_t)(bxy[u][0] & 0xffffu), by0 = (int16_t)(bxy[u][0] >> 16), bx1 = (int16_t)(bxy[u][1] & 0xffffu), by1 = (int16_t)(bxy[u][1] >> 16);
        const bool k = d < P.n_recs && (op != OP_DRAW || ((!shadow || (P.flags & kPickShadows)) && bx0 < tx0 + kPickTile && bx1 > tx0 &&
                                                          by0 < ty0 + kPickTile && by1 > ty0));
        const unsigned long long m = __ballot(k);
        if (lane == 0 && c0 + u < nch) keep[c0 + u] = m;
      }
    }
    __syncthreads();
    for (int c = 0; c < nch; c++) {
      const unsigned long long mv = keep[c];
      unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mv >> 32)) << 32) |
                             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mv);
      while (m) {
        const int d = w0 + c * 64 + __builtin_ctzll(m);
        m &= m - 1ull;
        while (d >= next_pf) {  // a new phase: its open clips are re-emitted as records of its own
          ph++;
          next_pf = ph + 1 < P.n_phases ? P.phase_first[ph + 1] : 0x7fffffff;
          depth = 0; mk = 1.0f; rm = 1.0f;
        }
        const DrawRec* rp = P.draws + d;
        const uint32_t om = rp->op_mode, op = (om >> 12) & 15u;
        if (op == OP_MASK_POP) {
          depth = max(depth - 1, 0);
          mk = depth > 0 ? (float)get(depth - 1) * inv255 : 1.0f;
          continue;
        }
        if (op == OP_RMASK_END) { rm = 1.0f; continue; }
        if (op == OP_RMASK_BEGIN) { rm = rect_mask_alpha(*rp, (float)px + 0.5f, (float)py + 0.5f); continue; }
        const bool inb = valid && px >= rp->bx0 && px < rp->bx1 && py >= rp->by0 && py < rp->by1;
        float a = 0.0f;
        if (inb) {
          const Src s = shade_one<true>(rp, P.exts, &P.atlas, nullptr, 0, false, px, py, opaque);
          a = s.covered ? s.a : 0.0f;
        }
        if (op == OP_MASK_PUSH) {  // mask.frag:186-234 drawn into a cleared R8 plane: stored = q8(a * a), a = shape * parent
          a *= mk;
          const float q = __builtin_rintf(a * a * 255.0f);
          put(depth, (uint32_t)q);
          depth++;
          mk = q * inv255;
          continue;
        }
        const float A = __builtin_rintf(255.0f * (a * mk * rm));
        if (inb && A >= thr) {
          if (kRegion) {
            last_draw = d;
          } else {
            P.hits[(size_t)pt * P.max_hits + (size_t)(n_hits % P.max_hits)] = make_uint2((uint32_t)d, (uint32_t)A | ((om & 255u) << 8));
            n_hits++;
          }
        }
      }
    }
  }
  if (kRegion) {
    if (in_rect) P.region_out[(size_t)(py - P.y0) * P.w + (size_t)(px - P.x0)] = valid ? last_draw : -1;
  } else if (pt >= 0) {
    P.hit_count[pt] = n_hits;
  }
}

void launch_pick(hipStream_t s, const PickParams& P, int n_groups, int spill_levels) {
  if (n_groups <= 0) return;
  if (P.region_out) hipLaunchKernelGGL(k_pick<true>, dim3(n_groups), dim3(kPickThreads), 0, s, P, spill_levels);
  else hipLaunchKernelGGL(k_pick<false>, dim3(n_groups), dim3(kPickThreads), 0, s, P, spill_levels);
}

}  // namespace fdh
