"""Top-k of a classifier's score rows on the device (include/dnn_hip_post.h: dnn_classify_topk,
csrc/classify.hip): per image the k largest entries in descending order, equal scores in ascending
index order.

    tk = TopK(batch, classes, k, device)
    tk.run(scores_ptr, n, stream)                  # asynchronous, [n, classes] fp32 on the device
    idx, score = tk.to_rows(tk.index[:n].cpu().numpy(), tk.score[:n].cpu().numpy(),
                            tk.status[:n].cpu().numpy())

status[i] is 0, or TOPK_NAN for a row that holds a NaN (that image's rows are not written); to_rows
raises for such an image unless raise_errors=False, which returns its rows as index -1, score NaN.
"""
import ctypes

import numpy as np

import dnn_hip

TOPK_MAX = 16   # DNN_TOPK_MAX
TOPK_NAN = -1   # DNN_TOPK_NAN
MAX_CLASSES = dnn_hip.SOFTMAX_MAX_CLASSES


def _bind(lib):
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.dnn_classify_topk.restype, lib.dnn_classify_topk.argtypes = i, [vp, i, i, i, vp, vp, vp, vp]
    lib.dnn_classify_topk_host.restype, lib.dnn_classify_topk_host.argtypes = i, [vp, i, i, i, vp, vp, vp]
    return lib


_lib = _bind(dnn_hip.mylib)


def _check_shape(classes, k):
    if not 1 <= classes <= MAX_CLASSES:
        raise ValueError(f"{classes} classes: 1..{MAX_CLASSES} expected")
    if not 1 <= k <= min(TOPK_MAX, classes):
        raise ValueError(f"k = {k}: 1..min({TOPK_MAX}, {classes} classes) expected")


def topk_host(scores, k):
    """(index [n, k] int32, score [n, k] fp32, status [n] int32) of host scores [n, classes]
    (dnn_classify_topk_host: copies in, runs the kernel, copies out).  Rows of an image with a
    non-zero status are index -1, score NaN."""
    x = np.ascontiguousarray(scores, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"scores {x.shape}: [n, classes] expected")
    n, classes = x.shape
    _check_shape(classes, k)
    index = np.full((n, k), -1, np.int32)
    score = np.full((n, k), np.nan, np.float32)
    status = np.zeros(n, np.int32)
    vp = dnn_hip._vp
    dnn_hip._check(_lib.dnn_classify_topk_host(vp(x), n, classes, int(k), vp(index), vp(score), vp(status)),
                   "dnn_classify_topk_host")
    return index, score, status


class TopK(object):
    """Device-side results for up to `batch` images (torch tensors on `device`): index [batch, k]
    int32, score [batch, k] fp32 and status [batch] int32, filled by `run(ptr, n, stream)`
    asynchronously from the [n, classes] fp32 rows at device address `ptr`."""

    def __init__(self, batch, classes, k, device):
        import torch
        _check_shape(int(classes), int(k))
        self.batch, self.classes, self.k = int(batch), int(classes), int(k)
        self.index = torch.full((self.batch, self.k), -1, dtype=torch.int32, device=device)
        self.score = torch.full((self.batch, self.k), float("nan"), dtype=torch.float32, device=device)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=device)

    def run(self, ptr, n, stream):
        if n > self.batch:
            raise ValueError(f"{n} images > the {self.batch} these buffers were sized for")
        dnn_hip._check(_lib.dnn_classify_topk(ptr, int(n), self.classes, self.k, self.index.data_ptr(),
                                              self.score.data_ptr(), self.status.data_ptr(), stream),
                       "dnn_classify_topk")

    @staticmethod
    def to_rows(index, score, status, raise_errors=True):
        """Host copies -> (index [n, k], score [n, k]); an image with a non-zero status raises
        ValueError, or with raise_errors=False gets index -1 and score NaN."""
        index, score = np.array(index, np.int32), np.array(score, np.float32)
        bad = np.flatnonzero(np.asarray(status) != 0)
        if len(bad) and raise_errors:
            raise ValueError(f"image {int(bad[0])}: its scores hold a NaN (status {int(np.asarray(status)[bad[0]])})")
        index[bad], score[bad] = -1, np.nan
        return index, score
