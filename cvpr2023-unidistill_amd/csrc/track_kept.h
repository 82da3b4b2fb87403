// The kept test of the tracking evaluation, section ROWS of ud_track_metric (include/unidistill_hip.h), stated once for the
// stages that need it (track_interp.hip).
#pragma once
#include "ud_common.h"

// candidate: the side's own precondition (predictions: track_id > 0; ground truth: gt_keep and gt_num_pts > 0).  vals[0 .. nvals)
// must be finite, vals[0] / vals[1] are x / y; ego: the sample's ego translation; range: metres per class.  A candidate of a tracked
// class with a non-finite value ORs nonfinite_bit into st and is not kept.
__device__ __forceinline__ bool ud_tm_row_kept(bool candidate, int c, int num_classes, const unsigned char* tracked,
                                               const double* range, const double* vals, int nvals, const double* ego,
                                               int nonfinite_bit, int& st) {
  if (!candidate || c < 0 || c >= num_classes || !tracked[c]) return false;
  bool finite = true;
  for (int i = 0; i < nvals; ++i) finite = finite && isfinite(vals[i]);
  if (!finite) {
    st |= nonfinite_bit;
    return false;
  }
  return ud_dist_xy(vals[0], vals[1], ego[0], ego[1]) <= range[c];
}
