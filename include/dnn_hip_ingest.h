/* dnn_hip_ingest.h — frame preprocessing on the GPU, exported by both libraries.
 *
 * Replaces the host `resize_input(im)` of the reference driver
 * (cs492-projects/proj3/__init__.py:8-12: cv2.resize to 416x416, / 255., BGR -> RGB,
 * float32) for a batch of frames already on the device, so a caller uploads 8-bit frames
 * (0.52 MB for a 416x416 frame instead of 2.08 MB of fp32) and the engine reads the fp32
 * NHWC tensor the reference would have produced.  The Python pipeline with pinned host
 * buffers and copy/compute overlap is dnn-inference-engine_amd/ingest.py.
 *
 * Resize: OpenCV's scalar fixed-point INTER_LINEAR for 8-bit images restated (11-bit
 * coefficients, see csrc/ingest.hip); parity with cv2 itself is unpinned (cv2 is not
 * importable in the build image).  /255, the channel order and the fp32 rounding are exact.
 */
#ifndef DNN_HIP_INGEST_H
#define DNN_HIP_INGEST_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* d_bgr: [n][h][w][3] uint8 BGR (device); d_out: [n][out_h][out_w][3] fp32 RGB in [0, 1]
 * (device); asynchronous on `stream` (hipStream_t, NULL = default). */
int dnn_preprocess_frames(const uint8_t* d_bgr, int n, int h, int w, float* d_out, int out_h, int out_w,
                          void* stream);

/* ---- letterbox ingest: what a Darknet-trained model expects ------------------------------
 * The reference stretches a frame to the network's size (above).  The original Darknet keeps the
 * aspect: letterbox_image resizes to the largest size of the image's aspect that fits, with
 * resize_image's two bilinear passes, and embeds the result centred in a 0.5 canvas; load_image
 * scales bytes by 1 / 255.  These entries restate that for a batch of uint8 images of DIFFERENT
 * sizes (csrc/letterbox.hip has the arithmetic, tests/letterbox_oracle.py restates it in numpy).
 * Darknet's source is not readable in the build image, so parity with a Darknet binary is
 * unpinned; the geometry, / 255, the channel order and every fp32 rounding of the stated
 * arithmetic are exact.  Darknet's last-row rule is kept: for some size pairs the last resized
 * row is nearly black (16 rows -> 96 rows is one).
 *
 * Error channel: 0 ok, nonzero with a message in dnn_last_error(); bad arguments (NULL pointers,
 * n < 0, a non-positive size, a network input of 2^31 floats or more, an unknown order, a frame
 * past pixels_bytes, a letterbox with a side below 2 pixels: the message names the frame) return
 * before any device call. */

/* one frame of a ragged batch: h x w x 3 bytes at `offset` of the pixel buffer, rows contiguous */
typedef struct dnn_frame {
  unsigned long long offset;
  int h, w;
} dnn_frame;

#define DNN_PIXELS_BGR 0 /* cv2 frames: flipped to RGB, as dnn_preprocess_frames does */
#define DNN_PIXELS_RGB 1 /* taken as it is */

/* letterbox_image's size rule.  Host only: no device is touched.
 *   if (float)net_w / src_w < (float)net_h / src_h:  new_w = net_w, new_h = (src_h * net_w) / src_w
 *   else:                                            new_h = net_h, new_w = (src_w * net_h) / src_h
 *   pad_x = (net_w - new_w) / 2, pad_y = (net_h - new_h) / 2      (integer divisions)
 * Nonzero when new_h or new_w is below 2 (resize_image divides by new - 1). */
int dnn_letterbox_geometry(int src_h, int src_w, int net_h, int net_w, int* new_h, int* new_w, int* pad_y,
                           int* pad_x);

/* letterbox_image + load_image's scaling for n frames.  d_pixels: pixels_bytes bytes on the
 * device holding the frames anywhere, in any order; frames: a HOST array of n descriptors, fully
 * read before the call returns; d_out: [n][net_h][net_w][3] fp32 RGB (device), 0.5 outside each
 * frame's image, every element written exactly once (no memset needed); order: DNN_PIXELS_*.
 * Asynchronous on `stream` (hipStream_t, NULL = default): no copy, no synchronisation. */
int dnn_letterbox_frames(const uint8_t* d_pixels, unsigned long long pixels_bytes, const dnn_frame* frames, int n,
                         float* d_out, int net_h, int net_w, int order, void* stream);

/* The same with host pointers, synchronous (allocates, copies in, runs, copies out). */
int dnn_letterbox_frames_host(const uint8_t* pixels, unsigned long long pixels_bytes, const dnn_frame* frames, int n,
                              float* out, int net_h, int net_w, int order);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
