// Rotated-BEV IoU and greedy NMS for the proposal layer (eval / predict_boxes_when_training path).
//
// Replaces `iou3d_nms_cuda.nms_gpu` (reference unidistill/layers/head/det3d/generate_proposals/
// centerpoint_gen_proposals.py:85-105; the extension binary is not in the reference tree -- it is the
// OpenPCDet iou3d_nms op, whose published behaviour is restated here): boxes are
// (x, y, z, dx, dy, dz, heading), already sorted by descending score; box i suppresses every later box
// j with BEV IoU(i, j) > thresh unless i itself was suppressed.  BEV footprint = dx x dy rectangle
// rotated by heading about (x, y).  Intersection = Sutherland-Hodgman clipping of rectangle A by the
// four half-planes of rectangle B, shoelace area; IoU = inter / max(area_a + area_b - inter, 1e-8).
//
//   k_nms_mask   : one thread per (box i, block of 64 later boxes) -> 64 suppression bits
//                  (nms_scan.h: ud_nms_mask_word)
//   k_nms_reduce : ONE wave walks the boxes in score order (nms_scan.h: ud_nms_scan; the inherently
//                  sequential part, kept on the device so the proposal layer never synchronises with
//                  the host); keep list and count are written out.
#include "ud_common.h"
#include "ud_prof.h"
#include "nms_scan.h"

namespace {

using ud_iou::iou_bev;

__global__ __launch_bounds__(256) void k_nms_mask(const float* __restrict__ boxes, int N, float thresh,
                                                  unsigned long long* __restrict__ mask, int words) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)N * words) return;
  const int i = (int)(t / words), wj = (int)(t - (long long)i * words);
  mask[(size_t)i * words + wj] = ud_nms_mask_word(boxes, 7, i, wj, N, thresh);
}

__global__ __launch_bounds__(64) void k_nms_reduce(const unsigned long long* __restrict__ mask, int N,
                                                   int words, long long* __restrict__ keep,
                                                   int* __restrict__ num_keep) {
  const int lane = threadIdx.x;
  const int count = ud_nms_scan<kNmsWordsPerLane>(
      mask, N, words, words, N, [&](int i, int k) { if (lane == 0) keep[k] = i; },
      [](int, int, unsigned long long) {});
  if (lane == 0) *num_keep = count;
  for (int k = count + lane; k < N; k += 64) keep[k] = -1;
}

__global__ __launch_bounds__(256) void k_iou_matrix(const float* __restrict__ a, int Na,
                                                    const float* __restrict__ b, int Nb,
                                                    float* __restrict__ iou) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)Na * Nb) return;
  const int i = (int)(t / Nb), j = (int)(t - (long long)i * Nb);
  float ba[7], bb[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { ba[k] = a[(size_t)i * 7 + k]; bb[k] = b[(size_t)j * 7 + k]; }
  iou[t] = iou_bev(ba, bb);
}

constexpr int kMaxBoxes = ud_nms_scan_capacity(kNmsWordsPerLane);   // 16384

}  // namespace

extern "C" {

size_t ud_nms_bev_workspace_bytes(int N) {
  if (N <= 0) return 0;
  const int words = (N + 63) / 64;
  return ud_align_up((size_t)N * words * sizeof(unsigned long long));
}

int ud_nms_rotated_bev(const float* boxes, int N, float thresh, long long* keep, int* num_keep,
                       void* workspace, size_t workspace_bytes, ud_stream_t stream_) {
  if (N < 0 || !num_keep) return UD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (N == 0) {
    UD_HIP_TRY(hipMemsetAsync(num_keep, 0, sizeof(int), stream));
    return UD_OK;
  }
  if (!boxes || !keep) return UD_ERR_INVALID_ARG;
  if (N > kMaxBoxes) return UD_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < ud_nms_bev_workspace_bytes(N)) return UD_ERR_WORKSPACE;
  const int words = (N + 63) / 64;
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(workspace);
  UdProfScope prof("nms.rotated_bev", stream);
  k_nms_mask<<<ud_div_up((long long)N * words, 256), 256, 0, stream>>>(boxes, N, thresh, mask, words);
  UD_LAUNCH_CHECK();
  k_nms_reduce<<<1, 64, 0, stream>>>(mask, N, words, keep, num_keep);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

int ud_boxes_iou_bev(const float* a, int Na, const float* b, int Nb, float* iou, ud_stream_t stream_) {
  if (Na < 0 || Nb < 0) return UD_ERR_INVALID_ARG;
  if (Na == 0 || Nb == 0) return UD_OK;
  if (!a || !b || !iou) return UD_ERR_INVALID_ARG;
  k_iou_matrix<<<ud_div_up((long long)Na * Nb, 256), 256, 0, (hipStream_t)stream_>>>(a, Na, b, Nb, iou);
  UD_LAUNCH_CHECK();
  return UD_OK;
}

}  // extern "C"
