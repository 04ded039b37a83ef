// k_damage_codec.hip -- coded damage readback (include/figdraw_hip_stream.h, which specifies the format): k_damage_encode codes each
// pending bin losslessly -- SOLID, PAL, RUNS or RAW, whichever payload is smallest -- and stores directory entry and payload straight into
// page-locked host memory.  One launch; the shape of k_damage_pack (k_damage.hip).
#include "fdh_device.h"
#include "fdh_damage.h"

namespace fdh {

constexpr int kEncThreads = 256;
constexpr int kEncPerThread = kBin * kBin / kEncThreads;  // 16 pixels of the tight order per thread
constexpr int kEncSlots = 1024;                           // the colour set: open addressing, at most 512 slots are ever taken
constexpr int kEncMaxColours = 256;
constexpr uint32_t kEncEmpty = 0xFFFFFFFFu;               // an empty slot; the COLOUR of that value is kept in a flag instead
constexpr int kEncRunsPerThread = (kBin * kBin * 4 / 6 + kEncThreads - 1) / kEncThreads;  // RUNS is chosen for 6 n <= 4 w h only

struct EncShared {
  uint32_t buf[kBin * kBin];       // the tile, tight; then the payload as it will lie in the blob
  uint32_t key[kEncSlots];         // the colour set
  uint16_t rank[kEncSlots];        // PAL: the index of a slot's colour
  uint32_t list[kEncMaxColours];   // the set's colours in order of arrival, and their slots
  uint16_t slot_of[kEncMaxColours];
  uint32_t part[kEncThreads / 64];
  uint32_t n_colours, has_empty, offset;
};

__device__ __forceinline__ uint32_t enc_hash(uint32_t c) { return (c * 0x9E3779B1u) >> 22; }

// Colour c joins the set.  Gives up once more than kEncMaxColours have arrived: every thread then has at most one insertion under way,
// so no more than 2 * kEncMaxColours slots are taken and a probe always meets an empty one.
__device__ __forceinline__ void enc_insert(EncShared& S, uint32_t c) {
  if (c == kEncEmpty) { S.has_empty = 1u; return; }
  uint32_t slot = enc_hash(c);
  for (;;) {
    if (*(volatile uint32_t*)&S.n_colours > (uint32_t)kEncMaxColours) return;
    const uint32_t old = atomicCAS(&S.key[slot], kEncEmpty, c);
    if (old == c) return;
    if (old == kEncEmpty) {
      const uint32_t k = atomicAdd(&S.n_colours, 1u);
      if (k < (uint32_t)kEncMaxColours) { S.list[k] = c; S.slot_of[k] = (uint16_t)slot; }
      return;
    }
    slot = (slot + 1) & (kEncSlots - 1);
  }
}
// the index of a colour that is in the set (n: the palette's size)
__device__ __forceinline__ uint32_t enc_index(const EncShared& S, uint32_t c, uint32_t n) {
  if (c == kEncEmpty) return n - 1;  // the largest value there is
  uint32_t slot = enc_hash(c);
  while (S.key[slot] != c) slot = (slot + 1) & (kEncSlots - 1);
  return S.rank[slot];
}

// a thread's 16 pixels as indices of B bits each: 16 B bits from bit 0 of word[0] on (a pixel inside a run has its predecessor's index)
template <int B>
__device__ __forceinline__ void enc_pack(const EncShared& S, const uint32_t (&px)[kEncPerThread], int nv, uint32_t starts, uint32_t n_col,
                                         uint32_t (&word)[4]) {
  uint32_t cur = 0;
#pragma unroll
  for (int j = 0; j < kEncPerThread; j++) {
    if (j < nv) {
      if (j == 0 || ((starts >> j) & 1u)) cur = enc_index(S, px[j], n_col);
      word[(j * B) >> 5] |= cur << ((j * B) & 31);
    }
  }
}

__global__ __launch_bounds__(kEncThreads) void k_damage_encode(const DamageEncodeParams P) {
  __shared__ __attribute__((aligned(16))) EncShared S;
  const int nb = P.bins_x * P.bins_y;
  const int bin = (int)blockIdx.x, t = (int)threadIdx.x;
  if (bin >= nb) return;
  uint32_t slot_dir;
  if (!pending_slot<kEncThreads, true>(P.stamp, P.epoch, P.all, bin, nb, P.n_tiles, S.part, slot_dir)) return;
  const TileBox box = tile_box(bin, P.bins_x, P.W, P.H);
  const int x0 = box.x0, y0 = box.y0, w = box.w, h = box.h;
  const int n_px = w * h;

  // 1. the tile, tight, into LDS
  const bool rows_aligned = (P.W & 3) == 0;
  tile_walk<kEncThreads>(P.surf, P.W, box, [&](int, int r, int c, bool inside, const uint32_t* __restrict__ src) {
    if (!inside) return;
    uint32_t* d = S.buf + r * w + c;
    if (rows_aligned && w == kBin) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(src);
    else {
      d[0] = src[0];
      if (c + 1 < w) d[1] = src[1];
      if (c + 2 < w) d[2] = src[2];
      if (c + 3 < w) d[3] = src[3];
    }
  });
  if (t == 0) { S.n_colours = 0; S.has_empty = 0; }
  __syncthreads();

  // each thread's 16 pixels of the tight order, in registers from here on: S.buf becomes the payload
  const int base = t * kEncPerThread;
  const int nv = min(max(n_px - base, 0), kEncPerThread);
  uint32_t px[kEncPerThread];
  if (nv == kEncPerThread) {
#pragma unroll
    for (int q = 0; q < kEncPerThread / 4; q++) {
      const uint4 v = reinterpret_cast<const uint4*>(S.buf + base)[q];
      px[4 * q] = v.x; px[4 * q + 1] = v.y; px[4 * q + 2] = v.z; px[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kEncPerThread; j++) px[j] = j < nv ? S.buf[base + j] : 0u;
  }
  const uint32_t before = (t > 0 && nv > 0) ? S.buf[base - 1] : 0u;

  // 2. run starts over the tight order: bit j of `starts`
  uint32_t starts = 0;
#pragma unroll
  for (int j = 0; j < kEncPerThread; j++) {
    const bool st = j < nv && (base + j == 0 || px[j] != (j ? px[j - 1] : before));
    starts |= (st ? 1u : 0u) << j;
  }
  const uint32_t my_runs = (uint32_t)__popc(starts);
  uint32_t incl = my_runs;  // the workgroup's prefix sum: this thread's first start is run `first_run`
#pragma unroll
  for (int sh = 1; sh < 64; sh <<= 1) {
    const uint32_t o = __shfl_up(incl, sh, 64);
    if ((t & 63) >= sh) incl += o;
  }
  if ((t & 63) == 63) S.part[t >> 6] = incl;
  // (the colour set's slots are emptied under the same barrier)
#pragma unroll
  for (int k = 0; k < kEncSlots / kEncThreads; k++) S.key[t + k * kEncThreads] = kEncEmpty;
  __syncthreads();
  uint32_t n_runs = 0, first_run = incl - my_runs;
#pragma unroll
  for (int wv = 0; wv < kEncThreads / 64; wv++) {
    const uint32_t p = S.part[wv];
    if (wv < (t >> 6)) first_run += p;
    n_runs += p;
  }

  // 3. the distinct colours, when PAL can win at all: its smallest payload is two colours and a bit per pixel, and RUNS wins a tie
  // against nothing below it
  const uint32_t raw_size = 4u * (uint32_t)n_px;
  const uint32_t runs_size = 4u * ((6u * n_runs + 3u) / 4u);
  const bool try_pal = n_runs > 1 && 8u + 4u * (((uint32_t)n_px + 31u) / 32u) <= min(runs_size, raw_size);
  uint32_t n_col = 0, bits = 0, pal_size = 0xFFFFFFFFu;
  if (try_pal) {  // (uniform)
    uint32_t m = starts;
    while (m) {  // a colour enters the set where a run of it starts
      const int j = __ffs(m) - 1;
      m &= m - 1;
      uint32_t c = px[0];
#pragma unroll
      for (int q = 1; q < kEncPerThread; q++) c = q == j ? px[q] : c;
      enc_insert(S, c);
    }
    __syncthreads();
    if (S.n_colours <= (uint32_t)kEncMaxColours && S.n_colours + S.has_empty <= (uint32_t)kEncMaxColours) {
      n_col = S.n_colours + S.has_empty;
      bits = n_col <= 2 ? 1u : n_col <= 4 ? 2u : n_col <= 16 ? 4u : 8u;
      pal_size = 4u * n_col + 4u * (((uint32_t)n_px * bits + 31u) / 32u);
    }
  }

  // 4. the mode: the smallest payload, ties to the lower number
  uint32_t mode = 3, size = raw_size;
  if (runs_size <= size) { mode = 2; size = runs_size; }
  if (pal_size <= size) { mode = 1; size = pal_size; }
  if (n_runs == 1) { mode = 0; size = 0; }
  const uint32_t claim = (size + 15u) & ~15u;

  // 5. its space in the blob
  // (one 64-bit add: the bytes claimed so far in bits 0 .. 39, the claims made above them; whoever makes the last one knows the blob's end)
  if (t == 0) {
    const unsigned long long old = atomicAdd(P.cursor, (unsigned long long)claim | 1ull << 40);
    const uint32_t at = (uint32_t)(old & ((1ull << 40) - 1ull));
    S.offset = claim ? at : 0u;
    if ((uint32_t)(old >> 40) + 1u == P.n_pending) P.payload_bytes[0] = at + claim;
  }

  // 6. the payload, in S.buf (every thread has read its pixels: the barrier after the colour set's, or the one above)
  if (mode == 1) {
    const uint32_t n_tab = S.n_colours;
    if ((uint32_t)t < n_tab) {  // a colour's index is the number of colours below it
      const uint32_t c = S.list[t];
      uint32_t r = 0;
      for (uint32_t k = 0; k < n_tab; k++) r += S.list[k] < c ? 1u : 0u;
      S.rank[S.slot_of[t]] = (uint16_t)r;
      S.buf[r] = c;
    }
    if (t == 0 && S.has_empty) S.buf[n_col - 1] = kEncEmpty;
    __syncthreads();
    const uint32_t n_words = ((uint32_t)n_px * bits + 31u) / 32u;
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (bits == 1) enc_pack<1>(S, px, nv, starts, n_col, word);
    else if (bits == 2) enc_pack<2>(S, px, nv, starts, n_col, word);
    else if (bits == 4) enc_pack<4>(S, px, nv, starts, n_col, word);
    else enc_pack<8>(S, px, nv, starts, n_col, word);
    uint32_t* idx = S.buf + n_col;
    if (bits == 1) {  // 16 pixels are half a word
      if ((uint32_t)t < 2u * n_words) reinterpret_cast<uint16_t*>(idx)[t] = (uint16_t)word[0];
    } else {
      const uint32_t per = bits / 2u;  // words per thread: 1, 2, 4
#pragma unroll
      for (uint32_t q = 0; q < 4; q++)
        if (q < per && (uint32_t)t * per + q < n_words) idx[(uint32_t)t * per + q] = word[q];
    }
  } else if (mode == 2) {
    __syncthreads();  // (no barrier since the pixels were read when the colour set was not tried)
    uint16_t* pos = reinterpret_cast<uint16_t*>(S.buf + n_runs);  // first each run's start, then its length - 1
    uint32_t m = starts, r = first_run;
    while (m) {
      const int j = __ffs(m) - 1;
      m &= m - 1;
      uint32_t c = px[0];
#pragma unroll
      for (int q = 1; q < kEncPerThread; q++) c = q == j ? px[q] : c;
      S.buf[r] = c;
      pos[r] = (uint16_t)(base + j);
      r++;
    }
    __syncthreads();
    uint16_t len[kEncRunsPerThread];
#pragma unroll
    for (int k = 0; k < kEncRunsPerThread; k++) {
      const uint32_t i = (uint32_t)t + (uint32_t)k * kEncThreads;
      len[k] = i < n_runs ? (uint16_t)((i + 1 < n_runs ? (uint32_t)pos[i + 1] : (uint32_t)n_px) - (uint32_t)pos[i] - 1u) : (uint16_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kEncRunsPerThread; k++) {
      const uint32_t i = (uint32_t)t + (uint32_t)k * kEncThreads;
      if (i < n_runs) pos[i] = len[k];
    }
    if (t == 0 && (n_runs & 1u)) pos[n_runs] = 0;  // the padding to 4 bytes
  }
  __syncthreads();
  if ((uint32_t)t < (claim - size) / 4u) S.buf[size / 4u + (uint32_t)t] = 0u;  // the round-up to 16 bytes is zeros
  __syncthreads();

  // 7. out: payload (16 bytes per thread and step, consecutive) and entry
  const uint32_t offset = S.offset;
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(P.payload + offset);
  for (uint32_t v = (uint32_t)t; v < claim / 16u; v += kEncThreads) dst[v] = reinterpret_cast<const uint4*>(S.buf)[v];
  if (t == 0) {
    uint2* e = P.dir + (size_t)slot_dir * 3;
    e[0] = make_uint2((uint32_t)x0 | (uint32_t)y0 << 16, (uint32_t)w | (uint32_t)h << 16);
    e[1] = make_uint2(mode | (mode == 1 ? bits : 0u) << 8 | (mode == 1 ? n_col : mode == 2 ? n_runs : 0u) << 16, offset);
    e[2] = make_uint2(size, mode == 0 ? px[0] : 0u);
  }
}

void launch_damage_encode(hipStream_t s, const DamageEncodeParams& P) {
  const int nb = P.bins_x * P.bins_y;
  if (nb <= 0) return;
  FDH_LAUNCH(k_damage_encode, dim3(nb), dim3(kEncThreads), 0, s, P);
}

}  // namespace fdh
