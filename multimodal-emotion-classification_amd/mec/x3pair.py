"""Host re-layout of fp32x3 hi / lo planes between the planar and the paired form.

A split tensor X[rows][K] (K % 32 == 0) is two f16 planes, hi and lo. Paired, it is one f16 array
[rows][2K] holding, for every 32-element K chunk, the chunk's hi halfs followed by its lo halfs, so one
row's operands of one 32-deep K step are one aligned 128-byte line (csrc/mec_common.h x3_pair_index,
include/mec.h mec_gemm_f16x3_paired). Values are untouched; only addresses move.
"""
import torch

CHUNK = 32


def pair_index(r, k, K, plane):
    """Flat index of element (r, k) of `plane` (0 hi, 1 lo) in the paired array of a [rows][K] tensor."""
    return r * 2 * K + (k >> 5) * 64 + plane * 32 + (k & 31)


def pair(hi, lo):
    """hi, lo: [rows, K] -> paired [rows, 2K] (a new contiguous tensor)."""
    rows, K = hi.shape
    if hi.shape != lo.shape or K % CHUNK:
        raise ValueError('pair: planes of one shape [rows, K] with K % 32 == 0')
    both = torch.stack((hi.reshape(rows, K // CHUNK, CHUNK), lo.reshape(rows, K // CHUNK, CHUNK)), dim=2)
    return both.reshape(rows, 2 * K).contiguous()


def unpair(x):
    """paired [rows, 2K] -> (hi, lo), each [rows, K] contiguous."""
    rows, K2 = x.shape
    if K2 % (2 * CHUNK):
        raise ValueError('unpair: [rows, 2K] with K % 32 == 0')
    both = x.reshape(rows, K2 // (2 * CHUNK), 2, CHUNK)
    K = K2 // 2
    return both[:, :, 0, :].reshape(rows, K).contiguous(), both[:, :, 1, :].reshape(rows, K).contiguous()
