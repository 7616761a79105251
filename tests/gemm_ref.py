"""Float64 host references and shapes shared by the kernel-level GEMM-mode tests
(test_gpu_gemm_modes.py); the references are themselves checked against torch's float64 conv2d on
the CPU (test_host.py), so a wrong reference can neither pass nor fail a kernel."""
import numpy as np

# (n, H, W, C, Cout, ks, stride, pad): the smallest geometries that still hit each addressing case
GEOMETRIES = {
    'G1': (3, 7, 7, 64, 64, 3, 1, 1),       # M = 147: one partial tile spanning three images
    'G2': (2, 9, 14, 128, 128, 3, 2, 1),    # H != W, odd H at stride 2 (OH 5, OW 7), two K chunks per tap
    'G3': (5, 15, 15, 64, 128, 3, 2, 1),    # M = 320: several M tiles, partial last one at BM 128 and 256
    'G4': (2, 10, 6, 128, 64, 1, 2, 0),     # strided 1x1, non-square, M = 30
    'G5': (1, 20, 20, 64, 256, 3, 1, 1),    # N = 256: the 256-wide tiles take part
}


def out_extent(H, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1


def tap_view(x, kh, kw, ks, stride, pad):
    """x[n, oh s - p + kh, ow s - p + kw, c] for every output (oh, ow), 0 where that is padding:
    what a conv whose only nonzero weights sit at tap (kh, kw) reads. x: [n, H, W, C]."""
    n, H, W, C = x.shape
    OH, OW = out_extent(H, ks, stride, pad), out_extent(W, ks, stride, pad)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    return xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]


def conv_nhwc_f64(x, w, stride, pad):
    """NHWC conv in float64: x [n, H, W, C], w [Cout, ks, ks, C] -> [n, OH, OW, Cout], as the sum over
    the filter taps of (tap view of x) . w[:, kh, kw, :]^T."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    ks = w.shape[1]
    out = 0.0
    for kh in range(ks):
        for kw in range(ks):
            out = out + tap_view(x, kh, kw, ks, stride, pad) @ w[:, kh, kw, :].T
    return out


def dual_gather(a2, stride):
    """The A_DUAL second source as a matrix: a2 [n, H, W, C] read at (oh stride, ow stride), 1x1
    unpadded -> [n OH OW, C]."""
    g = tap_view(a2, 0, 0, 1, stride, 0)
    return np.ascontiguousarray(g).reshape(-1, a2.shape[3])
