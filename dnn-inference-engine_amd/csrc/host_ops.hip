// The join / element-wise kernels on host tensors (include/dnn_hip_plan.h: dnn_spp_host,
// dnn_route_host, dnn_shortcut_host, dnn_scale_shift_host, dnn_upsample_host, dnn_slice_host).  Host code only:
// each entry checks its arguments and hands on_device() its inputs and a launch.
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <vector>
#include "dnn_common.h"
#include "plan_internal.h"
#include "../../include/dnn_hip_plan.h"

using namespace dnnhip;

namespace {

struct HostTensor {
  const float* host;  // NULL: nothing to upload (its device slot is still there)
  size_t floats;
};

constexpr int kMaxInputs = 3;

// One device allocation holding every input (64-float aligned) and `scratch` floats behind them;
// uploads the inputs, calls launch(d, &result) with d[i] input i's device address and d[ins.size()]
// the scratch's (the launch sets `result` to where its output lies), downloads out_floats from
// there and frees the allocation.
template <class Launch>
int on_device(const char* who, std::initializer_list<HostTensor> ins, size_t scratch, float* out, size_t out_floats,
              Launch launch) {
  size_t off[kMaxInputs + 1], total = 0;
  int k = 0;
  for (const HostTensor& t : ins) {
    off[k++] = total;
    total += align_up(t.floats, 64);
  }
  off[k] = total;
  float* base = nullptr;
  DNN_HIP_TRY(hipMalloc(&base, (total + scratch) * sizeof(float)));
  float* d[kMaxInputs + 1];
  for (int i = 0; i <= k; ++i) d[i] = base + off[i];
  int rc = 0, i = 0;
  for (const HostTensor& t : ins) {
    if (t.host && t.floats && hipMemcpy(d[i], t.host, t.floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("%s: host to device copy failed", who);
      rc = -1;
      break;
    }
    ++i;
  }
  const float* result = nullptr;
  if (!rc) rc = launch(d, &result);
  if (!rc && hipMemcpy(out, result, out_floats * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("%s: device to host copy failed (%s)", who, hipGetErrorString(hipGetLastError()));
    rc = -1;
  }
  (void)hipFree(base);
  return rc;
}

constexpr unsigned long long k2GiB = 0x80000000ULL;

}  // namespace

extern "C" {

int dnn_spp_host(const float* a, float* out, int n, int h, int w, int c, int n_sizes, const int* sizes, int x_first) {
  DNN_REQUIRE(a && out, "dnn_spp_host: NULL tensor");
  DNN_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "dnn_spp_host: bad shape n=%d %dx%dx%d", n, h, w, c);
  if (int rc = spp_sizes_ok("dnn_spp_host", n_sizes, sizes)) return rc;
  if (n == 0) return 0;
  const size_t af = (size_t)n * h * w * c, of = af * (n_sizes + 1);
  DNN_REQUIRE(of * 4 < k2GiB, "dnn_spp_host: the output of n=%d %dx%dx%d with %d sizes is >= 2 GiB; split the batch",
              n, h, w, c, n_sizes);
  return on_device("dnn_spp_host", {{a, af}}, of, out, of, [&](float* const* d, const float** res) {
    *res = d[1];
    return launch_spp(d[0], d[1], n, h, w, c, n_sizes, sizes, x_first, nullptr);
  });
}

int dnn_route_host(const float* a, const float* b, float* out, int n, int h, int w, int ca, int block, int cb,
                   int b_first) {
  DNN_REQUIRE(a && out, "dnn_route_host: NULL tensor");
  DNN_REQUIRE(n >= 0 && h > 0 && w > 0 && ca > 0 && cb >= 0, "dnn_route_host: bad shape n=%d %dx%dx%d cb=%d", n, h, w,
              ca, cb);
  DNN_REQUIRE(block >= 1 && block <= 8, "dnn_route_host: block %d outside 1..8", block);
  DNN_REQUIRE(h % block == 0 && w % block == 0, "dnn_route_host: %dx%d input is not a multiple of block %d", h, w,
              block);
  DNN_REQUIRE((b != nullptr) == (cb > 0), "dnn_route_host: b must be NULL exactly when cb == 0");
  if (n == 0) return 0;
  const size_t pix = (size_t)n * (h / block) * (w / block);
  const size_t af = (size_t)n * h * w * ca, bf = pix * cb, of = pix * ((size_t)block * block * ca + cb);
  DNN_REQUIRE(af * 4 < k2GiB && bf * 4 < k2GiB && of * 4 < k2GiB,
              "dnn_route_host: a tensor of n=%d %dx%dx%d block %d cb=%d is >= 2 GiB; split the batch", n, h, w, ca,
              block, cb);
  return on_device("dnn_route_host", {{a, af}, {b, bf}}, of, out, of, [&](float* const* d, const float** res) {
    *res = d[2];
    return launch_route(d[0], bf ? d[1] : nullptr, d[2], n, h, w, ca, block, cb, b_first, nullptr);
  });
}

int dnn_shortcut_host(const float* a, const float* b, float* out, int n, int h, int w, int c, int leaky) {
  DNN_REQUIRE(a && b && out, "dnn_shortcut_host: NULL tensor");
  DNN_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "dnn_shortcut_host: bad shape n=%d %dx%dx%d", n, h, w, c);
  DNN_REQUIRE(leaky >= 0 && leaky <= 2, "dnn_shortcut_host: leaky must be 0, 1 or 2");
  if (n == 0) return 0;
  const size_t f = (size_t)n * h * w * c;
  DNN_REQUIRE(f * 4 < k2GiB, "dnn_shortcut_host: a tensor of n=%d %dx%dx%d is >= 2 GiB; split the batch", n, h, w, c);
  return on_device("dnn_shortcut_host", {{a, f}, {b, f}}, f, out, f, [&](float* const* d, const float** res) {
    *res = d[2];
    return launch_shortcut(d[0], d[1], d[2], (long long)f, leaky, nullptr);
  });
}

int dnn_scale_shift_host(const float* a, const float* scale, const float* shift, float* out, int n, int h, int w,
                         int c, int leaky) {
  DNN_REQUIRE(a && out, "dnn_scale_shift_host: NULL tensor");
  DNN_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "dnn_scale_shift_host: bad shape n=%d %dx%dx%d", n, h, w, c);
  DNN_REQUIRE((scale == nullptr) == (shift == nullptr), "dnn_scale_shift_host: scale and shift must be both set or both NULL");
  DNN_REQUIRE(leaky >= 0 && leaky <= 2, "dnn_scale_shift_host: leaky must be 0, 1 or 2");
  DNN_REQUIRE(scale || leaky, "dnn_scale_shift_host: nothing to do (no scale / shift and no leaky)");
  if (n == 0) return 0;
  const size_t f = (size_t)n * h * w * c;
  DNN_REQUIRE(f * 4 < k2GiB, "dnn_scale_shift_host: a tensor of n=%d %dx%dx%d is >= 2 GiB; split the batch", n, h, w,
              c);
  std::vector<float> beta(c);
  for (int k = 0; k < c; ++k) beta[k] = scale ? -shift[k] : 0.f;  // v * alpha - beta, beta = -shift (exact)
  return on_device("dnn_scale_shift_host", {{a, f}, {scale, (size_t)c}, {scale ? beta.data() : nullptr, (size_t)c}}, f,
                   out, f, [&](float* const* d, const float** res) {
                     int rc = 0;
                     *res = d[0];  // the two kernels ping-pong between the input's slot and the scratch
                     if (scale) {
                       rc = launch_bn_ab(d[0], d[1], d[2], d[3], (long long)f, c, nullptr);
                       *res = d[3];
                     }
                     if (!rc && leaky) {
                       float* dst = *res == d[0] ? d[3] : d[0];
                       rc = launch_leaky(*res, dst, (long long)f, leaky == 2 ? 1 : 0, nullptr);
                       *res = dst;
                     }
                     return rc;
                   });
}

int dnn_upsample_host(const float* a, float* out, int n, int h, int w, int c, int factor) {
  DNN_REQUIRE(a && out, "dnn_upsample_host: NULL tensor");
  DNN_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "dnn_upsample_host: bad shape n=%d %dx%dx%d", n, h, w, c);
  DNN_REQUIRE(factor >= 1 && factor <= 8, "dnn_upsample_host: factor %d outside 1..8", factor);
  if (n == 0) return 0;
  const size_t af = (size_t)n * h * w * c;
  DNN_REQUIRE(af * 4 < k2GiB && af * factor * factor * 4 < k2GiB,
              "dnn_upsample_host: the output of n=%d %dx%dx%d factor %d is >= 2 GiB; split the batch", n, h, w, c,
              factor);
  const size_t of = af * factor * factor;
  return on_device("dnn_upsample_host", {{a, af}}, of, out, of, [&](float* const* d, const float** res) {
    *res = d[1];
    return launch_upsample(d[0], d[1], n, h, w, c, factor, nullptr);
  });
}

int dnn_slice_host(const float* a, float* out, int n, int h, int w, int c, int first, int channels) {
  DNN_REQUIRE(a && out, "dnn_slice_host: NULL tensor");
  DNN_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "dnn_slice_host: bad shape n=%d %dx%dx%d", n, h, w, c);
  DNN_REQUIRE(first >= 0 && channels >= 1 && (long long)first + channels <= c,
              "dnn_slice_host: first %d, channels %d outside the tensor's %d channels", first, channels, c);
  if (n == 0) return 0;
  const size_t af = (size_t)n * h * w * c, of = (size_t)n * h * w * channels;
  DNN_REQUIRE(af * 4 < k2GiB, "dnn_slice_host: a tensor of n=%d %dx%dx%d is >= 2 GiB; split the batch", n, h, w, c);
  return on_device("dnn_slice_host", {{a, af}}, of, out, of, [&](float* const* d, const float** res) {
    *res = d[1];
    return launch_slice(d[0], d[1], n, h, w, c, first, channels, nullptr);
  });
}

}  // extern "C"
