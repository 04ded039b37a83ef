// tests/emu/selftest.cpp -- toy kernels that hold the two host shims to their own contract (tests/test_emu_shim_host.py copies a shim beside
// this file as fdh_device.h; -DEMU_THREADS: it is the threaded one).  usage: selftest CASE -> "ok", exit 0; a wrong answer: a line, exit 1;
// the cases named lane_leaves_*, wave_alone_* and waves_disagree are defects the sequential shim must end with exit code 4.
#include "fdh_device.h"
#include <cstdio>
#include <cstring>
#include <vector>
#define CHECK(what) do { if (!(what)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #what); return 1; } } while (0)

#ifndef EMU_THREADS
#ifndef FDH_MSDF_ANY  // as the kernels have it: without a wave the lane's own word is the answer
#define FDH_MSDF_ANY(p) (p)
#endif
static int flat_block() { return blockIdx.y * gridDim.x + blockIdx.x; }
__global__ void k_ballot(unsigned long long* out, int* geometry, int leaver) {
  const int t = threadIdx.x, at = flat_block() * blockDim.x + t;
  if (t == leaver) return;
  const unsigned long long first = __ballot((t & 63) % 3 == 0);
  out[2 * at] = first;
  out[2 * at + 1] = __ballot((t & 63) % 3 == 0);
  int* g = geometry + 6 * at;
  g[0] = blockIdx.x; g[1] = blockIdx.y; g[2] = gridDim.x; g[3] = gridDim.y; g[4] = blockDim.x; g[5] = blockDim.y;
}
__global__ void k_barrier(int* out, int leaver) {
  __shared__ int slot[256];
  HIP_DYNAMIC_SHARED(int, dyn)
  const int t = threadIdx.x, n = blockDim.x;
  slot[t] = t; dyn[t] = 1000 * flat_block() + t;
  if (t == leaver) return;
  __syncthreads();
  out[flat_block() * n + t] = slot[n - 1 - t] + dyn[n - 1 - t];
}
__global__ void k_votes(int* out) {
  const int t = threadIdx.x, n = blockDim.x;
  const bool group_yes = FDH_IMAGE_SDF_GROUP_ANY(t == n - 56), group_no = FDH_IMAGE_SDF_GROUP_ANY(false);  // (lane 200 of 256)
  const bool wave_no = FDH_IMAGE_SDF_WAVE_ANY(false), wave_yes = FDH_IMAGE_SDF_WAVE_ANY((t & 63) == 63);
  out[flat_block() * n + t] = group_yes | group_no << 1 | wave_no << 2 | wave_yes << 3;
}
__global__ void k_wave_alone_at_a_vote(int) {
  if (threadIdx.x >> 6 == 1) FDH_IMAGE_SDF_GROUP_ANY(true);
}
__global__ void k_waves_disagree(int) {
  if (threadIdx.x >> 6 == 1) FDH_IMAGE_SDF_WAVE_ANY(true);
  __syncthreads();
}
__global__ void k_any(int* out) { out[threadIdx.x] = FDH_MSDF_ANY(threadIdx.x % 3 == 0) ? 1 : 0; }

static int ballots(int n_lanes) {
  const dim3 grid(2, 2), block(n_lanes);
  const int n = 4 * n_lanes, n_waves = n_lanes / 64;
  std::vector<unsigned long long> out(2 * n, 0);
  std::vector<int> geometry(6 * n, -1);
  FDH_LAUNCH(k_ballot, grid, block, 0, nullptr, out.data(), geometry.data(), -1);
  for (int i = 0; i < n; i++) {
    CHECK(out[2 * i] == 0x9249249249249249ull && out[2 * i + 1] == 0x9249249249249249ull);
    const int b = i / n_lanes, want[6] = {b % 2, b / 2, 2, 2, n_lanes, 1};
    CHECK(!memcmp(&geometry[6 * i], want, sizeof want));
  }
  // two ballots a wave: three passes a workgroup, one round a wave
  CHECK(emu::workgroups == 4 && emu::lanes == n && emu::passes == 12 && emu::ballots == 8 * n_waves && emu::rounds == 4 * n_waves && emu::workgroups_with_rounds == 4);
  return 0;
}
static int barrier(int n_lanes) {
  const dim3 grid(2, 2), block(n_lanes);
  std::vector<int> out(4 * n_lanes, -1);
  FDH_LAUNCH(k_barrier, grid, block, n_lanes * sizeof(int), nullptr, out.data(), -1);  // (under AddressSanitizer: the block holds n_lanes ints)
  for (int i = 0; i < 4 * n_lanes; i++) CHECK(out[i] == 2 * (n_lanes - 1 - i % n_lanes) + 1000 * (i / n_lanes));
  CHECK(emu::workgroups == 4 && emu::passes == 8 && emu::ballots == 0 && emu::rounds == 0 && emu::workgroups_with_rounds == 0);
  return 0;
}
static int votes(int n_lanes) {
  const dim3 grid(2, 2), block(n_lanes);
  std::vector<int> out(4 * n_lanes, -1);
  FDH_LAUNCH(k_votes, grid, block, 0, nullptr, out.data());
  for (int v : out) CHECK(v == (1 | 0 << 1 | 0 << 2 | 1 << 3));
  CHECK(emu::workgroups == 4 && emu::ballots == 8 * (n_lanes / 64) && emu::rounds == 4 * (n_lanes / 64));
  return 0;
}
static int any() {
  int out[64];
  FDH_LAUNCH(k_any, dim3(1), dim3(64), 0, nullptr, out);
  for (int t = 0; t < 64; t++) {
#ifdef EMU_LANES_ALONE
    CHECK(out[t] == (t % 3 == 0));
#else
    CHECK(out[t] == 1);
#endif
  }
  return 0;
}
static int run(const char* c) {
  std::vector<unsigned long long> masks(2 * 256);
  std::vector<int> ints(6 * 256);
  if (!strcmp(c, "ballots_64")) return ballots(64);
  if (!strcmp(c, "ballots_256")) return ballots(256);
  if (!strcmp(c, "barrier_64")) return barrier(64);
  if (!strcmp(c, "barrier_256")) return barrier(256);
  if (!strcmp(c, "votes_64")) return votes(64);
  if (!strcmp(c, "votes_256")) return votes(256);
  if (!strcmp(c, "any")) return any();
  if (!strcmp(c, "lane_leaves_before_a_ballot")) FDH_LAUNCH(k_ballot, dim3(1), dim3(64), 0, nullptr, masks.data(), ints.data(), 5);
  if (!strcmp(c, "lane_leaves_before_a_barrier")) FDH_LAUNCH(k_barrier, dim3(1), dim3(256), 1024, nullptr, ints.data(), 70);
  if (!strcmp(c, "wave_alone_at_a_vote")) FDH_LAUNCH(k_wave_alone_at_a_vote, dim3(1), dim3(128), 0, nullptr, 0);
  if (!strcmp(c, "waves_disagree")) FDH_LAUNCH(k_waves_disagree, dim3(1), dim3(128), 0, nullptr, 0);
  return 2;  // (not reached by the four above)
}
#else
struct Params { uint32_t* out; uint32_t* counter; unsigned long long* total; };
__global__ void k_threads(const Params P) {
  __shared__ uint32_t slot[256];
  const uint32_t t = threadIdx.x;
  uint32_t* o = P.out + 5 * (blockIdx.x * 256 + t);
  o[0] = __shfl_xor(t, 1, 64);
  o[1] = __shfl_up(t, 3, 64);
  unsigned long long mask = 0;
  if (t >> 6 == 1) mask = __ballot((t & 63) % 3 == 0);  // a branch only wave 1 takes
  o[2] = (uint32_t)mask; o[3] = (uint32_t)(mask >> 32);
  slot[t] = t;
  __syncthreads();
  o[4] = slot[255 - t] + gridDim.x;
  atomicAdd(P.counter, 1u);
  atomicAdd(P.total, (unsigned long long)t);
}
static int run(const char* c) {
  if (strcmp(c, "threads")) return 2;
  const int grid = 4;
  std::vector<uint32_t> out(5 * 256 * grid, 0xEEEEEEEEu);
  uint32_t counter = 0;
  unsigned long long total = 0;
  const Params P{out.data(), &counter, &total};
  FDH_LAUNCH(k_threads, dim3(grid), dim3(256), 0, nullptr, P);
  for (uint32_t i = 0; i < 256u * grid; i++) {
    const uint32_t t = i % 256, *o = &out[5 * i];
    CHECK(o[0] == (t ^ 1u) && o[1] == ((t & 63) >= 3 ? t - 3 : t));
    CHECK(o[2] == (t >> 6 == 1 ? 0x49249249u : 0u) && o[3] == (t >> 6 == 1 ? 0x92492492u : 0u));
    CHECK(o[4] == 255 - t + grid);
  }
  CHECK(counter == 256u * grid && total == 255ull * 128 * grid);
  return 0;
}
#endif
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int r = run(argv[1]);
  if (!r) printf("ok\n");
  return r;
}
