"""Frame ingest: host uint8 BGR frames -> the engine's fp32 NHWC input on the GPU
(the reference's `resize_input`, cs492-projects/proj3/__init__.py:8-12).

`resize_input_gpu(im)` is the drop-in for one frame (returns the numpy array the reference
returns).  `FrameIngest` is the batched pipeline: frames are copied into one of two pinned
host buffers, uploaded as 8-bit data on a copy stream (4x fewer PCIe bytes than fp32), then
resized / scaled / channel-flipped on the GPU (`dnn_preprocess_frames`,
include/dnn_hip_ingest.h) on the compute stream, so the upload of batch k+1 overlaps the
forward of batch k.  No CPU fallback: the library must be present.

The reference stretches a frame to the network's size.  A Darknet-trained model expects a
letterbox instead: the image resized with its aspect kept, centred in a 0.5 canvas
(`dnn_letterbox_frames`; the arithmetic is in csrc/letterbox.hip).  `letterbox_gpu(im)` is the
one-image call, `RaggedIngest` the same two-slot pipeline for batches of images of DIFFERENT
sizes; `yolo_post.DetectionBuffers.correct` maps the decoded boxes back into each image's own
pixels.
"""
import collections
import ctypes

import numpy as np

import dnn_hip

_lib = dnn_hip.mylib
_lib.dnn_preprocess_frames.restype = ctypes.c_int
_lib.dnn_preprocess_frames.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p]


class Frame(ctypes.Structure):
    """dnn_frame (include/dnn_hip_ingest.h): h x w x 3 bytes at `offset` of the pixel buffer."""
    _fields_ = [("offset", ctypes.c_ulonglong), ("h", ctypes.c_int), ("w", ctypes.c_int)]


_ip = ctypes.POINTER(ctypes.c_int)
_lib.dnn_letterbox_geometry.restype = ctypes.c_int
_lib.dnn_letterbox_geometry.argtypes = [ctypes.c_int] * 4 + [_ip] * 4
_lib.dnn_letterbox_frames.restype = ctypes.c_int
_lib.dnn_letterbox_frames.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.POINTER(Frame), ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
_lib.dnn_letterbox_frames_host.restype = ctypes.c_int
_lib.dnn_letterbox_frames_host.argtypes = _lib.dnn_letterbox_frames.argtypes[:-1]

IN_SIZE = 416
PIXEL_ORDERS = {"bgr": 0, "rgb": 1}  # DNN_PIXELS_BGR, DNN_PIXELS_RGB


def preprocess_device(d_bgr_ptr, n, h, w, d_out_ptr, stream_ptr, out_hw=(IN_SIZE, IN_SIZE)):
    dnn_hip._check(_lib.dnn_preprocess_frames(d_bgr_ptr, int(n), int(h), int(w), d_out_ptr, int(out_hw[0]),
                                              int(out_hw[1]), stream_ptr), "dnn_preprocess_frames")


def resize_input_gpu(im, device=0):
    """__init__.py:8-12 for one HxWx3 uint8 BGR frame -> [416,416,3] fp32 RGB (numpy)."""
    import torch
    im = np.ascontiguousarray(im, dtype=np.uint8)
    if im.ndim != 3 or im.shape[2] != 3:
        raise ValueError(f"expected an HxWx3 uint8 BGR frame, got shape {im.shape}")
    dev = torch.device("cuda", device)
    src = torch.from_numpy(im).to(dev)
    out = torch.empty((IN_SIZE, IN_SIZE, 3), dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev)
    preprocess_device(src.data_ptr(), 1, im.shape[0], im.shape[1], out.data_ptr(), s.cuda_stream)
    return out.cpu().numpy()


class FrameIngest(object):
    """Double-buffered uint8 upload + GPU preprocessing for batches of `batch` frames of
    h x w x 3 uint8 BGR.  submit(frames) returns the fp32 [n,416,416,3] device tensor for
    that batch; it is ready in stream order on `compute_stream`.

    Slot reuse is ordered without any call from the caller: before slot k is refilled,
      * the host waits until the previous upload out of pinned host[k] has completed
        (next_host_buffer / submit_host), so the CPU never rewrites a buffer the copy
        engine is still reading;
      * the copy stream waits for the previous preprocess that read dev_u8[k], so an upload
        never overwrites 8-bit frames that are still being resized;
      * the preprocess writing out[k] runs on the compute stream after everything enqueued
        there before it (the forward that read out[k] two batches ago).
    release(stream) is needed only when the returned tensor is consumed on ANOTHER stream:
    it records that consumption so the preprocess that next overwrites the slot waits for it."""

    def __init__(self, batch, h, w, device, compute_stream=None, out_hw=(IN_SIZE, IN_SIZE)):
        import torch
        self.torch = torch
        self.batch, self.h, self.w, self.out_hw = int(batch), int(h), int(w), tuple(out_hw)
        self.dev = torch.device(device) if not isinstance(device, torch.device) else device
        shape = (self.batch, self.h, self.w, 3)
        self.host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev_u8 = [torch.empty(shape, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self.out = [torch.empty((self.batch,) + self.out_hw + (3,), dtype=torch.float32, device=self.dev)
                    for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(self.dev)
        self.compute = compute_stream or torch.cuda.current_stream(self.dev)
        self.uploaded = [None, None]   # upload out of host[k] (copy stream)
        self.prepped = [None, None]    # preprocess that read dev_u8[k] (compute stream)
        self.consumed = [None, None]   # off-stream consumer of out[k] (release())
        self.slot = 0
        self.last = None

    def next_host_buffer(self):
        """The pinned uint8 [batch, h, w, 3] buffer the next submit_host() uploads: a frame
        decoder can write into it directly (no extra host copy).  Waits (host) until the
        previous upload out of that buffer has completed."""
        if self.uploaded[self.slot] is not None:
            self.uploaded[self.slot].synchronize()
        return self.host[self.slot]

    def submit(self, frames):
        """frames: [n, h, w, 3] uint8 BGR (numpy), n <= batch: copied into the next pinned
        slot, then submit_host(n)."""
        f = np.asarray(frames, dtype=np.uint8)
        n = f.shape[0]
        if n > self.batch or f.shape[1:] != (self.h, self.w, 3):
            raise ValueError(f"frames of shape {f.shape} do not fit [{self.batch},{self.h},{self.w},3]")
        self.next_host_buffer()[:n].numpy()[...] = f
        return self.submit_host(n)

    def submit_host(self, n):
        """Upload the first n frames of the current pinned slot and preprocess them."""
        torch = self.torch
        if not 0 <= n <= self.batch:  # (before the slot flips: a rejected call changes nothing)
            raise ValueError(f"n={n} outside [0, {self.batch}]")
        k = self.slot
        self.slot ^= 1
        up = torch.cuda.Event()
        with torch.cuda.stream(self.copy_stream):
            if self.prepped[k] is not None:
                self.copy_stream.wait_event(self.prepped[k])  # dev_u8[k]'s last reader is done
            self.dev_u8[k][:n].copy_(self.host[k][:n], non_blocking=True)
            up.record(self.copy_stream)
        self.uploaded[k] = up
        self.compute.wait_event(up)
        if self.consumed[k] is not None:
            self.compute.wait_event(self.consumed[k])  # an off-stream reader of out[k]
            self.consumed[k] = None
        preprocess_device(self.dev_u8[k].data_ptr(), n, self.h, self.w, self.out[k].data_ptr(),
                          self.compute.cuda_stream, self.out_hw)
        pe = torch.cuda.Event()
        pe.record(self.compute)
        self.prepped[k] = pe
        self.last = k
        return self.out[k][:n]

    def release(self, stream=None):
        """The most recently returned batch is being read on `stream` (default: the compute
        stream, where nothing needs recording): call after that work has been enqueued, so
        the preprocess that reuses the slot waits for it.  Optional on the compute stream."""
        if self.last is None:
            return
        if stream is None or stream == self.compute:
            return
        e = self.torch.cuda.Event()
        e.record(stream)
        self.consumed[self.last] = e


# ------------------------------------------------------------------------- letterbox ingest
Letterbox = collections.namedtuple("Letterbox", "new_h new_w pad_y pad_x")


def letterbox_geometry(src_h, src_w, net_h, net_w):
    """Darknet's letterbox_image size rule (dnn_letterbox_geometry): the src_h x src_w image
    becomes new_h x new_w at (pad_y, pad_x) of the net_h x net_w input.  ValueError where a side
    comes out below 2 pixels or a size is not positive."""
    out = [ctypes.c_int(0) for _ in range(4)]
    if _lib.dnn_letterbox_geometry(int(src_h), int(src_w), int(net_h), int(net_w), *[ctypes.byref(o) for o in out]):
        raise ValueError(dnn_hip.last_error())
    return Letterbox(*[o.value for o in out])


def _order(order):
    if not isinstance(order, str) or order not in PIXEL_ORDERS:
        raise ValueError(f"order {order!r}: need one of {sorted(PIXEL_ORDERS)}")
    return PIXEL_ORDERS[order]


def letterbox_device(d_pixels_ptr, pixels_bytes, frames, n, d_out_ptr, stream_ptr, net_hw=(IN_SIZE, IN_SIZE),
                     order="bgr"):
    """dnn_letterbox_frames: `frames` a ctypes array of Frame (host), the pointers device."""
    dnn_hip._check(_lib.dnn_letterbox_frames(d_pixels_ptr, int(pixels_bytes), frames, int(n), d_out_ptr,
                                             int(net_hw[0]), int(net_hw[1]), _order(order), stream_ptr),
                   "dnn_letterbox_frames")


def ragged_layout(images, batch, max_bytes, net_hw):
    """Check a list of H x W x 3 uint8 images against a `batch` / `max_bytes` budget and the
    net_hw letterbox, and lay them back to back: (arrays, Frame array, [(h, w), ...], bytes).
    Host only; raises ValueError (wrong dtype or rank, too many images or bytes, a letterbox with
    a side below 2 pixels) and touches nothing."""
    images = list(images)
    if len(images) > batch:
        raise ValueError(f"{len(images)} images > batch {batch}")
    arrays, sizes, at = [], [], 0
    frames = (Frame * max(len(images), 1))()
    for i, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"image {i}: an H x W x 3 uint8 array expected, got "
                             f"{getattr(im, 'dtype', type(im).__name__)} of shape {getattr(im, 'shape', None)}")
        h, w = int(im.shape[0]), int(im.shape[1])
        if h < 1 or w < 1:
            raise ValueError(f"image {i}: size {h} x {w}")
        try:
            letterbox_geometry(h, w, net_hw[0], net_hw[1])
        except ValueError as e:
            raise ValueError(f"image {i}: {e}")
        frames[i] = Frame(at, h, w)
        arrays.append(im)
        sizes.append((h, w))
        at += 3 * h * w
    if at > max_bytes:
        raise ValueError(f"{at} pixel bytes > max_bytes {max_bytes}")
    return arrays, frames, sizes, at


def letterbox_gpu(im, net_hw=(IN_SIZE, IN_SIZE), order="bgr", device=0):
    """Darknet's letterbox_image for one H x W x 3 uint8 image -> [net_h, net_w, 3] fp32 RGB
    (numpy); order "bgr" (cv2 frames, flipped) or "rgb"."""
    import torch
    _order(order)
    arrays, frames, _, nbytes = ragged_layout([im], 1, 1 << 62, net_hw)
    dev = torch.device("cuda", device)
    src = torch.from_numpy(np.ascontiguousarray(arrays[0])).to(dev)
    out = torch.empty(tuple(net_hw) + (3,), dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev)
    letterbox_device(src.data_ptr(), nbytes, frames, 1, out.data_ptr(), s.cuda_stream, net_hw, order)
    return out.cpu().numpy()


class RaggedIngest(object):
    """FrameIngest for images of any sizes: up to `batch` H x W x 3 uint8 images and `max_bytes`
    pixel bytes per submit, laid back to back in one of two pinned host buffers, uploaded as 8-bit
    data on a copy stream, then letterboxed into the fp32 [n, net_h, net_w, 3] tensor on the
    compute stream (dnn_letterbox_frames).  submit(images) returns that tensor, ready in stream
    order on `compute_stream`, and the images' (h, w) list, which
    yolo_post.DetectionBuffers.correct takes.

    Slot reuse follows FrameIngest's three rules: the host waits for the previous upload out of
    pinned host[k] before rewriting it; the copy stream waits for the letterbox that last read
    dev_u8[k]; the letterbox writing out[k] runs on the compute stream after everything enqueued
    there before it.  release(stream) has FrameIngest's meaning: needed only when the returned
    tensor is consumed on ANOTHER stream.  A rejected submit raises before the slot flips and
    changes nothing."""

    def __init__(self, batch, max_bytes, net_hw=(IN_SIZE, IN_SIZE), device=0, compute_stream=None, order="bgr"):
        import torch
        self.torch = torch
        self.batch, self.max_bytes, self.net_hw = int(batch), int(max_bytes), (int(net_hw[0]), int(net_hw[1]))
        _order(order)
        self.order = order
        if self.batch < 1 or self.max_bytes < 1 or self.net_hw[0] < 1 or self.net_hw[1] < 1:
            raise ValueError(f"batch {batch}, max_bytes {max_bytes}, net_hw {net_hw}: positive sizes expected")
        self.dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.host = [torch.empty(self.max_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev_u8 = [torch.empty(self.max_bytes, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self.out = [None, None]        # fp32 [batch, net_h, net_w, 3], made by the first submit that returns it
        self.copy_stream = torch.cuda.Stream(self.dev)
        self.compute = compute_stream or torch.cuda.current_stream(self.dev)
        self.uploaded = [None, None]   # upload out of host[k] (copy stream)
        self.prepped = [None, None]    # letterbox that read dev_u8[k] (compute stream)
        self.consumed = [None, None]   # off-stream consumer of out[k] (release())
        self.slot = 0
        self.last = None

    def submit(self, images, out_ptr=None):
        """images: a list of H x W x 3 uint8 arrays, len <= batch, 3 * sum(H * W) <= max_bytes.
        Returns (tensor [n, net_h, net_w, 3], [(h, w), ...]).  With `out_ptr` (a device pointer
        to room for n frames, e.g. a plan's input buffer) the letterbox writes there instead of
        the slot's own tensor and the first value is None."""
        torch = self.torch
        arrays, frames, sizes, nbytes = ragged_layout(images, self.batch, self.max_bytes, self.net_hw)
        n = len(arrays)  # (everything above raises before the slot flips)
        k = self.slot
        self.slot ^= 1
        if self.uploaded[k] is not None:
            self.uploaded[k].synchronize()  # the copy engine is done reading host[k]
        host = self.host[k].numpy()
        for f, a in zip(frames, arrays):
            host[f.offset:f.offset + a.size] = a.reshape(-1)
        up = torch.cuda.Event()
        with torch.cuda.stream(self.copy_stream):
            if self.prepped[k] is not None:
                self.copy_stream.wait_event(self.prepped[k])  # dev_u8[k]'s last reader is done
            if nbytes:
                self.dev_u8[k][:nbytes].copy_(self.host[k][:nbytes], non_blocking=True)
            up.record(self.copy_stream)
        self.uploaded[k] = up
        self.compute.wait_event(up)
        if self.consumed[k] is not None:
            self.compute.wait_event(self.consumed[k])  # an off-stream reader of out[k]
            self.consumed[k] = None
        if out_ptr is None and self.out[k] is None:
            self.out[k] = torch.empty((self.batch,) + self.net_hw + (3,), dtype=torch.float32, device=self.dev)
        dst = self.out[k].data_ptr() if out_ptr is None else int(out_ptr)
        letterbox_device(self.dev_u8[k].data_ptr(), nbytes, frames, n, dst, self.compute.cuda_stream, self.net_hw,
                         self.order)
        pe = torch.cuda.Event()
        pe.record(self.compute)
        self.prepped[k] = pe
        self.last = k
        return (self.out[k][:n] if out_ptr is None else None), sizes

    def release(self, stream=None):
        """The most recently returned batch is being read on `stream` (default: the compute
        stream, where nothing needs recording): call after that work has been enqueued, so the
        letterbox that reuses the slot waits for it.  Optional on the compute stream."""
        if self.last is None:
            return
        if stream is None or stream == self.compute:
            return
        e = self.torch.cuda.Event()
        e.record(stream)
        self.consumed[self.last] = e
