// fdh_debug.cpp -- fault hunting: digests of what a frame recorded and of what the device was handed, surfaces read back.
#include "fdh_context.h"

#include <cstring>

namespace fdh {

// FNV-1a over the last frame's records in painter's order, in the form the calls produced them (four vertex colours, extension
// indices counted over the whole frame), their bounds, extensions and the phase table: two frames with equal digests hand the
// kernels identical input, however many threads recorded them.
uint64_t Context::record_digest() {
  drain();
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) { const uint8_t* b = static_cast<const uint8_t*>(p); for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
  const uint64_t n = frame_.n_records();
  mix(&n, sizeof n);
  uint32_t ext_base = 0;
  for (const Piece& p : frame_.pieces()) {
    const Lane& L = frame_.lane(p.lane);
    for (uint32_t i = 0; i < p.n; i++) {
      DrawRec r = L.recs[p.first + i];
      record_host_form(r);
      if (r.op_mode & F_GENERAL) r.ext = r.ext - p.ext_first + ext_base;
      mix(&r, sizeof r);
    }
    ext_base += p.n_ext;
  }
  for (const Piece& p : frame_.pieces()) { const Lane& L = frame_.lane(p.lane); for (uint32_t i = 0; i < p.n; i++) mix(&L.bins[p.first + i].box, sizeof(BBox)); }
  for (const Piece& p : frame_.pieces()) { const Lane& L = frame_.lane(p.lane); for (uint32_t i = 0; i < p.n_ext; i++) mix(&L.exts[p.ext_first + i], sizeof(QuadExt)); }
  for (const Phase& ph : frame_.phases()) { mix(&ph.first, sizeof ph.first); mix(&ph.count, sizeof ph.count); mix(&ph.blur, sizeof ph.blur); }
  return h;
}

// Fault hunting (fdh_debug_verify_upload): the device's frame block -- what k_upload_frame gathered for the frame last submitted --
// read back and compared with the lanes the records were made in (ordinary host memory, untouched until the staging set comes
// round again).  out[0..2] = bytes that differ in records / bin records / extensions, out[3] = bytes compared; out[4..9] describe the
// first difference: array (0, 1, 2), byte offset in the device array, the piece's lane, device dword, host dword, dwords of the
// device run that are zero; out[10] = pieces, out[11] = records.
void Context::debug_verify_upload(uint32_t out[24]) {
  need_device("debug_verify_upload");
  drain();
  FDH_HIP(hipSetDevice(device_));
  FDH_HIP(hipStreamSynchronize(stream_));
  for (int i = 0; i < 24; i++) out[i] = 0;
  const LaunchJob& J = job_;
  out[10] = (uint32_t)frame_.pieces().size(); out[11] = frame_.n_records();
  if (!J.dv.recs || frame_.n_records() == 0) return;
  std::vector<DrawRec> recs(frame_.n_records());
  std::vector<BinRec> bins(frame_.n_records());
  std::vector<QuadExt> exts(frame_.n_extensions());
  FDH_HIP(hipMemcpy(recs.data(), J.dv.recs, recs.size() * sizeof(DrawRec), hipMemcpyDeviceToHost));
  FDH_HIP(hipMemcpy(bins.data(), J.dv.binrecs, bins.size() * sizeof(BinRec), hipMemcpyDeviceToHost));
  if (!exts.empty()) FDH_HIP(hipMemcpy(exts.data(), J.dv.exts, exts.size() * sizeof(QuadExt), hipMemcpyDeviceToHost));
  bool first = true;
  auto cmp = [&](int array, int lane_no, const void* dev, const void* host, size_t bytes, size_t dev_off) {
    const uint32_t* d = static_cast<const uint32_t*>(dev);
    const uint32_t* h = static_cast<const uint32_t*>(host);
    out[3] += (uint32_t)bytes;
    for (size_t i = 0; i < bytes / 4; i++) {
      if (d[i] == h[i]) continue;
      out[array] += 4;
      if (first) {
        first = false;
        out[4] = (uint32_t)array; out[5] = (uint32_t)(dev_off + 4 * i); out[6] = (uint32_t)lane_no; out[7] = d[i]; out[8] = h[i];
        uint32_t z = 0;
        for (size_t k = 0; k < bytes / 4; k++) z += d[k] == 0u;
        out[9] = z;
      }
    }
  };
  uint32_t r0 = 0, e0 = 0;
  for (const Piece& p : frame_.pieces()) {
    const Lane& L = frame_.lane(p.lane);
    std::vector<DrawRec> want(L.recs.p + p.first, L.recs.p + p.first + p.n);
    for (DrawRec& r : want) if (r.op_mode & F_GENERAL) r.ext = r.ext - p.ext_first + e0;
    cmp(0, p.lane, recs.data() + r0, want.data(), (size_t)p.n * sizeof(DrawRec), (size_t)r0 * sizeof(DrawRec));
    cmp(1, p.lane, bins.data() + r0, L.bins.p + p.first, (size_t)p.n * sizeof(BinRec), (size_t)r0 * sizeof(BinRec));
    if (p.n_ext) cmp(2, p.lane, exts.data() + e0, L.exts.p + p.ext_first, (size_t)p.n_ext * sizeof(QuadExt), (size_t)e0 * sizeof(QuadExt));
    r0 += p.n; e0 += p.n_ext;
  }
  // the block from the chunk boxes on (chunk boxes, phase table, blur weight tables as far as this frame staged them): out[12] bytes
  // that differ, out[13] first offset (in that block), out[14] device dword, out[15] host dword, out[16] bytes compared
  {
    const size_t o_misc = J.layout.misc();
    std::vector<uint8_t> dev(misc_host_.size());
    if (!dev.empty()) FDH_HIP(hipMemcpy(dev.data(), d_frame_.ptr + o_misc, dev.size(), hipMemcpyDeviceToHost));
    out[16] = (uint32_t)dev.size();
    for (size_t i = 0; i + 4 <= dev.size(); i += 4) {
      uint32_t a, b;
      std::memcpy(&a, dev.data() + i, 4); std::memcpy(&b, misc_host_.data() + i, 4);
      if (a == b) continue;
      if (!out[12]) { out[13] = (uint32_t)i; out[14] = a; out[15] = b; }
      out[12] += 4;
    }
  }
  // the bin boxes the upload kernel derives from the bin records: out[17] boxes that differ from the host's, out[18] first index,
  // out[19] device value, out[20] host value
  {
    std::vector<uint32_t> box(frame_.n_records());
    FDH_HIP(hipMemcpy(box.data(), J.dv.binbox, box.size() * 4, hipMemcpyDeviceToHost));
    uint32_t g0 = 0;
    for (const Piece& p : frame_.pieces()) {
      const Lane& L = frame_.lane(p.lane);
      for (uint32_t i = 0; i < p.n; i++, g0++) {
        if (g0 == 0 && out[1]) continue;  // (a folded clear emptied record 0's box on the device side)
        if (box[g0] == L.boxes.p[p.first + i]) continue;
        if (!out[17]) { out[18] = g0; out[19] = box[g0]; out[20] = L.boxes.p[p.first + i]; }
        out[17]++;
      }
    }
  }
}

// Fault hunting (fdh_debug_bin_digest): what the bin kernel left for the frame last submitted -- per phase and bin the count and the
// list entries it covers.  out[0] = FNV-1a over them, out[1] = sum of the counts, out[2] = bins with count 0, out[3] = list entries
// whose first word is 0, out[4] = bins whose count exceeds the list stride (garbage).
void Context::debug_bin_digest(uint64_t out[8]) {
  need_device("debug_bin_digest");
  drain();
  FDH_HIP(hipSetDevice(device_));
  FDH_HIP(hipStreamSynchronize(stream_));
  for (int i = 0; i < 8; i++) out[i] = 0;
  const LaunchJob& J = job_;
  const size_t nb = (size_t)J.bins_x * J.bins_y, np = J.phases.size(), stride = (size_t)J.list_stride;
  if (!nb || !np || !J.counts || !J.lists) return;
  std::vector<uint32_t> counts(np * nb);
  std::vector<uint2> lists(np * nb * stride);
  FDH_HIP(hipMemcpy(counts.data(), J.counts, counts.size() * 4, hipMemcpyDeviceToHost));
  FDH_HIP(hipMemcpy(lists.data(), J.lists, lists.size() * sizeof(uint2), hipMemcpyDeviceToHost));
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint32_t v) { for (int k = 0; k < 4; k++) { h ^= (v >> (8 * k)) & 255u; h *= 1099511628211ull; } };
  for (size_t p = 0; p < np; p++) {
    const Phase& ph = J.phases[p];
    const bool whole = p == 0;
    for (int by = 0; by < J.bins_y; by++)
      for (int bx = 0; bx < J.bins_x; bx++) {
        if (!whole && (bx < ph.bin_x0 || bx >= ph.bin_x1 || by < ph.bin_y0 || by >= ph.bin_y1)) continue;  // (bins the phase's launches never look at)
        const size_t b = p * nb + (size_t)by * J.bins_x + bx;
        const uint32_t c = counts[b];
        mix(c);
        out[1] += c;
        if (c == 0) out[2]++;
        if (c > stride) { out[4]++; continue; }
        for (uint32_t e = 0; e < c; e++) { const uint2 v = lists[b * stride + e]; mix(v.x); mix(v.y); if (v.x == 0) out[3]++; }
      }
  }
  out[0] = h;
}

void Context::image_rect(int64_t key, int out_rect[4]) const {
  const AtlasEntry* e = atlas_.find(key);
  if (!e) throw Error(FDH_ERR_INVALID, "fdh_image_rect: unknown key");
  out_rect[0] = e->x; out_rect[1] = e->y; out_rect[2] = e->w; out_rect[3] = e->h;
}
void Context::debug_read_atlas_level(int level, uint8_t* out, int64_t capacity_bytes) {
  need_device("fdh_debug_read_atlas_level");
  if (level < 0 || level >= atlas_.n_levels()) throw Error(FDH_ERR_INVALID, "fdh_debug_read_atlas_level: the atlas has no such level");
  const size_t LS = (size_t)(atlas_.size() >> level), bytes = LS * LS * 4;
  if (capacity_bytes < (int64_t)bytes) throw Error(FDH_ERR_INVALID, "fdh_debug_read_atlas_level: the buffer is smaller than the level");
  sync();
  FDH_HIP(hipMemcpy(out, atlas_.level(level), bytes, hipMemcpyDeviceToHost));
}
void Context::debug_read_surface(int which, uint8_t* out) {
  need_device("debug_read_surface");
  drain();
  if (which == 4) {  // level 0 of the atlas, atlas_size x atlas_size
    FDH_HIP(hipSetDevice(device_));
    FDH_HIP(hipStreamSynchronize(stream_));
    FDH_HIP(hipMemcpy(out, atlas_.level0(), (size_t)atlas_.size() * atlas_.size() * 4, hipMemcpyDeviceToHost));
    return;
  }
  const uint32_t* src = which == 0 ? fb_ : which == 1 ? blur_tmp_ : which == 2 ? backdrop_ : which == 3 ? dbg_snap_ : nullptr;
  if (!src) throw Error(FDH_ERR_INVALID, "debug_read_surface: no such surface (or no frame yet)");
  FDH_HIP(hipSetDevice(device_));
  FDH_HIP(hipStreamSynchronize(stream_));
  FDH_HIP(hipMemcpy(out, src, (size_t)env_.W * env_.H * 4, hipMemcpyDeviceToHost));
}

}  // namespace fdh
