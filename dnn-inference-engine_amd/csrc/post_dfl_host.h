// The host side of the DFL decode (postprocess_dfl.hip defines it) for the entries that run it as their
// first phase: postprocess_dfl.hip's own and postprocess_seg.hip's.
#pragma once
#include "post_multi_dev.h"

namespace dnnhip {

struct DflCall {  // the arguments of an entry as its caller gave them (the host form: no workspace)
  const char* who;
  const dnn_yolo_dfl* h;
  const float* const* pred;
  int n_images;
  dnn_detection* dets;
  int max_det;
  int* counts;
  void* workspace;
  unsigned long long workspace_bytes;
  int nms_mode, labels_mode;
  int* points = nullptr;  // device, [n_images][max_det]: the grid point of every written row (postprocess_seg.hip)
};

// < 0 with the error set (it names the field), else the grid points of one image over all scales
int dfl_boxes(const dnn_yolo_dfl* h, const char* who);
// Every argument check, in the wide entries' order: the description, the modes, counts and pointers, pred[s],
// and unless `host` the workspace.  < 0 with the error set; 0 with nothing to do; 1 with *nb and *mp filled.
int check_dfl_call(const DflCall& c, bool host, int* nb, MultiPred* mp);
// The checks, then the three launches on `stream`.
int launch_yolo_dfl(const DflCall& c, hipStream_t stream);

}  // namespace dnnhip
