// Dataset preparation on the device (reference data/convert_endovis_to_coco.py:132-179, `np.unique(mask)`,
// `mask == class_id` and maskUtils.encode(np.asfortranarray(.)) per class, and data/apply_morphological_opening.py:
// 57-72, the encode after cv2.morphologyEx): the two steps between row-major bytes and the column-major bit words
// that s2h_rle_transitions (rle.hip) reads.  The index arithmetic is dataprep.h, shared with
// dataprep_host_check.cpp.
//
// s2h_label_hist: per frame the pixel count of every byte value.  A workgroup takes DP_HIST_CHUNK bytes of one
//   frame, a lane 16 consecutive bytes per step (one 16-byte load where the frame is 16-byte aligned), and
//   adds runs of equal bytes, not single bytes, to the workgroup's 256 32-bit counters in LDS -- a label
//   image is mostly long runs, so this is about one LDS atomic per lane and step.  The non-zero counters then go
//   to the frame's row with one global integer atomic each.  Integer adds only: the result does not depend on
//   their order.
// s2h_label_planes, staged (H <= DP_STAGED_MAX_H): a workgroup takes one frame and a band of 64 columns, loads
//   the band's H x 64 bytes row by row (16-byte loads where W is a multiple of 16) into the swizzled LDS tile of
//   dataprep.h, and then transposes from the tile: a wave takes 64 consecutive words of the band, lane l of
//   word w reads the byte at band position 64 w + l, and the 64 bytes a lane has read stay packed in 16
//   registers while every plane of the frame is built from them -- one ballot per word and plane, the ballot
//   of word i kept by lane i, so a wave stores its 64 words of a plane as one contiguous 512-byte row.  A
//   label byte leaves HBM once however many classes its frame holds.  A frame without planes loads nothing.
// s2h_label_planes, direct (taller images): one lane per column-major position reads its byte from global
//   memory (mask_export_kernel's mapping); lane 0 stores the ballot.
// Both forms write every word of every plane exactly once and nothing else; no 64-bit atomics, no float.
#include "common.h"
#include "dataprep.h"

namespace {

__global__ __launch_bounds__(DP_BLOCK) void label_hist_kernel(int HW, int nch, const uint8_t* labels, int* hist) {
  __shared__ int sh[256];
  sh[threadIdx.x] = 0;
  __syncthreads();
  const int f = blockIdx.x / nch, c = blockIdx.x - f * nch;
  const uint8_t* img = labels + (int64_t)f * HW;
  const bool vec = ((uintptr_t)img & 15) == 0;  // (offsets are multiples of 16)
#pragma unroll
  for (int s = 0; s < DP_HIST_STEPS; ++s) {
    const int o = dp_hist_offset(c, s, threadIdx.x);
    if (o >= HW) continue;
    const int n = HW - o < DP_HIST_LANE_BYTES ? HW - o : DP_HIST_LANE_BYTES;
    uint32_t q[4] = {0u, 0u, 0u, 0u};
    if (vec && n == DP_HIST_LANE_BYTES) {
      const uint4 v = *reinterpret_cast<const uint4*>(img + o);
      q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
    } else {
      for (int k = 0; k < n; ++k) q[k >> 2] |= (uint32_t)img[o + k] << (8 * (k & 3));
    }
    int cur = q[0] & 255, run = 0;
#pragma unroll
    for (int k = 0; k < DP_HIST_LANE_BYTES; ++k) {
      if (k < n) {
        const int v = (q[k >> 2] >> (8 * (k & 3))) & 255;
        if (v != cur) {
          atomicAdd(&sh[cur], run);
          cur = v;
          run = 0;
        }
        ++run;
      }
    }
    atomicAdd(&sh[cur], run);
  }
  __syncthreads();
  const int v = sh[threadIdx.x];
  if (v) atomicAdd(&hist[(int64_t)f * 256 + threadIdx.x], v);
}

__global__ __launch_bounds__(DP_BLOCK) void label_planes_staged_kernel(int H, int W, const uint8_t* labels, int P,
                                                                      const int* frame_off, const int* plane_class,
                                                                      uint64_t* bits, int nw) {
  extern __shared__ uint32_t tile[];  // dp_tile_dwords(H)
  const int nb = dp_bands(W);
  const int f = blockIdx.x / nb, b = blockIdx.x - f * nb;
  int p0, p1;
  dp_frame_planes(frame_off, f, P, &p0, &p1);
  if (p1 <= p0) return;  // (the same for every thread of the workgroup)
  const int cols = dp_band_cols(b, W);
  const uint8_t* img = labels + (int64_t)f * H * W + b * DP_BAND;
  const bool vec = (W & 15) == 0 && ((uintptr_t)labels & 15) == 0;  // then every segment start is 16-byte aligned
  for (int i = threadIdx.x; i < 4 * H; i += DP_BLOCK) {
    int r, seg;
    dp_load_item(i, &r, &seg);
    const int c0 = seg * 16;
    const uint8_t* src = img + (int64_t)r * W + c0;
    uint32_t q[4] = {0u, 0u, 0u, 0u};  // columns past the image stay zero
    if (vec && c0 + 16 <= cols) {
      const uint4 v = *reinterpret_cast<const uint4*>(src);
      q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
    } else {
      for (int k = 0; k < 16; ++k)
        if (c0 + k < cols) q[k >> 2] |= (uint32_t)src[k] << (8 * (k & 3));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[dp_tile_dword(r, seg * 4 + k)] = q[k];
  }
  __syncthreads();
  const uint8_t* t8 = reinterpret_cast<const uint8_t*>(tile);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nbw = dp_band_words(b, H, W), w0 = dp_band_word0(b, H);
  for (int base = wave * 64; base < nbw; base += (DP_BLOCK / 64) * 64) {
    uint32_t pk[16];    // byte i = this lane's pixel of word base + i
    uint64_t inm = 0;   // bit i: that pixel exists
#pragma unroll
    for (int i = 0; i < 16; ++i) pk[i] = 0u;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      int r, c;
      if (base + i < nbw && dp_word_pos(base + i, lane, H, cols, &r, &c)) {
        pk[i >> 2] |= (uint32_t)t8[dp_tile_byte(r, c)] << (8 * (i & 3));
        inm |= 1ull << i;
      }
    }
    const int w = base + lane;
    for (int p = p0; p < p1; ++p) {
      const int cls = plane_class[p];
      uint64_t keep = 0;
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        const int v = (pk[i >> 2] >> (8 * (i & 3))) & 255;
        const uint64_t m = __ballot(((inm >> i) & 1ull) && dp_bit(v, cls));
        if (lane == i) keep = m;
      }
      if (w < nbw && w0 + w < nw) bits[(int64_t)p * nw + w0 + w] = keep;
    }
  }
}

__global__ __launch_bounds__(DP_BLOCK) void label_planes_direct_kernel(int H, int W, const uint8_t* labels, int P,
                                                                      const int* frame_off, const int* plane_class,
                                                                      uint64_t* bits, int nw, int nblk) {
  const int f = blockIdx.x / nblk, blk = blockIdx.x - f * nblk;
  int p0, p1;
  dp_frame_planes(frame_off, f, P, &p0, &p1);
  if (p1 <= p0) return;
  const int HW = H * W;
  const int j = blk * DP_BLOCK + threadIdx.x;
  const bool in = j < HW;
  const int jj = in ? j : HW - 1;  // lanes past the end read the last pixel and contribute nothing
  const int x = jj / H, y = jj - x * H;
  const int v = labels[(int64_t)f * HW + (int64_t)y * W + x];
  const int lane = threadIdx.x & 63, word = j >> 6;  // the same word for the 64 lanes of a wave
  for (int p = p0; p < p1; ++p) {
    const uint64_t m = __ballot(in && dp_bit(v, plane_class[p]));
    if (lane == 0 && word < nw) bits[(int64_t)p * nw + word] = m;
  }
}

}  // namespace

extern "C" int s2h_label_hist(int F, int H, int W, const uint8_t* labels, int* hist, hipStream_t st) {
  const int64_t total = dp_total(F, H, W);
  if (total < 0) return (int)hipErrorInvalidValue;
  if (F == 0) return 0;
  if (!labels || !hist) return (int)hipErrorInvalidValue;
  s2h_zero_f32((float*)hist, 1, (int64_t)F * 256, (int64_t)F * 256, st);  // (int 0 = 0.0f bits)
  const int nch = dp_hist_chunks(H * W);  // (F * nch <= F H W / DP_HIST_CHUNK + F < 2^31)
  hipLaunchKernelGGL(label_hist_kernel, dim3((unsigned)((int64_t)F * nch)), dim3(DP_BLOCK), 0, st, H * W, nch, labels,
                     hist);
  S2H_LAUNCH_CHECK();
}

extern "C" int s2h_label_planes(int F, int H, int W, const uint8_t* labels, int P, const int* frame_off,
                                const int* plane_class, uint64_t* bits, hipStream_t st) {
  if (dp_total(F, H, W) < 0 || dp_total(P, H, W) < 0) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  if (F == 0 || !labels || !frame_off || !plane_class || !bits) return (int)hipErrorInvalidValue;
  const int nw = dp_words(H, W);
  if (dp_staged(H)) {
    const int lds = dp_tile_dwords(H) * 4;
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(label_planes_staged_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return (int)e;
    }
    // (F * bands <= F W < 2^31)
    hipLaunchKernelGGL(label_planes_staged_kernel, dim3((unsigned)((int64_t)F * dp_bands(W))), dim3(DP_BLOCK), lds, st,
                       H, W, labels, P, frame_off, plane_class, bits, nw);
  } else {
    const int nblk = (H * W + DP_BLOCK - 1) / DP_BLOCK;  // (F * nblk <= F H W / 256 + F < 2^31)
    hipLaunchKernelGGL(label_planes_direct_kernel, dim3((unsigned)((int64_t)F * nblk)), dim3(DP_BLOCK), 0, st, H, W,
                       labels, P, frame_off, plane_class, bits, nw, nblk);
  }
  S2H_LAUNCH_CHECK();
}
