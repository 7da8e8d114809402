"""``module1.Encoder.forward`` at inference on libapseq.so (csrc/seq/seq_encoder.hip): the pose network's self-attention encoder
(d_model 64, two heads, d_ff 2048, two layers and a closing Norm over one segment of up to 512 windows) as two launches per layer
instead of the library's chain of small ones -- ``apq_enc_qkv`` (Norm_1 and the three projections) and ``apq_enc_attn_ff`` (attention,
out-projection, residual, Norm_2, feed-forward, residual; the last layer's launch applies the encoder's closing Norm at its store).
The embedding and the positional term stay with the library: one ``addmm`` and one fused multiply-add.

Opt-in (``module1.set_encoder_backend('hip')``, ``APAMD_MODULE1_ENCODER=hip``, ``end2end --module1_encoder hip``); ``module1.Encoder``
decides who runs.  The weights are read where the module keeps them: nothing is packed or cached."""
import ctypes
import math

import torch

from . import _seqapi as Q
from . import ops


def _layer_tensors(layer):
    """the 16 parameter tensors of an EncoderLayer in the order the two calls take them, contiguous"""
    a, f = layer.attn, layer.ff
    ts = (layer.norm_1.alpha, layer.norm_1.bias, a.q_linear.weight, a.q_linear.bias, a.k_linear.weight, a.k_linear.bias,
          a.v_linear.weight, a.v_linear.bias, a.out.weight, a.out.bias, layer.norm_2.alpha, layer.norm_2.bias,
          f.linear_1.weight, f.linear_1.bias, f.linear_2.weight, f.linear_2.bias)
    return [t.detach().contiguous() for t in ts]


def _qkv_args(layer, lt, x, q, k, v, b, t, d):
    """the arguments of apq_enc_qkv_ok; x, q, k, v are c_void_p"""
    return [x, ops._ptr(lt[0]), ops._ptr(lt[1]), layer.norm_1.eps] + [ops._ptr(p) for p in lt[2:8]] + [q, k, v, b, t, d]


def _attn_args(layer, lt, final, x, q, k, v, y, b, t, d):
    """the arguments of apq_enc_attn_ff_ok; ``final``: the closing Norm's (alpha, bias) behind the last layer, else None"""
    fa, fb = (ops._ptr(final[0]), ops._ptr(final[1])) if final is not None else (None, None)
    return ([x, q, k, v] + [ops._ptr(p) for p in lt[8:12]] + [layer.norm_2.eps] + [ops._ptr(p) for p in lt[12:16]] +
            [fa, fb, final[2] if final is not None else 0.0, y, b, t, d, layer.attn.h, layer.ff.linear_1.out_features])


def _final(encoder):
    return encoder.norm.alpha.detach().contiguous(), encoder.norm.bias.detach().contiguous(), encoder.norm.eps


def supported(encoder, x):
    """What ``encoder_forward`` serves: a float32 CUDA batch (B, T, in_size) of a ``module1.Encoder`` with at least one layer and
    T within the positional table -- and the library's own word on the sizes and pointers of every layer (apq_enc_qkv_ok /
    apq_enc_attn_ff_ok: host only).  Who may call it (no mask, no gradients) is ``module1.Encoder.forward``'s business."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] >= 1 and x.shape[1] >= 1 and
            len(encoder.layers) >= 1 and x.shape[2] == encoder.embed.embed.in_features and x.shape[1] <= encoder.pe.pe.shape[1]):
        return False
    b, t, _ = x.shape
    d = encoder.pe.d_model
    lib = Q.lib()
    # encoder_forward allocates the activations and the workspace itself: torch's allocations are aligned far beyond what the
    # kernels ask, so an aligned stand-in address speaks for them
    fresh = ctypes.c_void_p(Q.ALIGN_WIDE)
    final = _final(encoder)
    if not all(p.is_cuda and p.dtype == torch.float32 and tuple(p.shape) == (d,) for p in final[:2]):
        return False
    for layer in encoder.layers:
        lt = _layer_tensors(layer)
        d_ff = layer.ff.linear_1.out_features
        shapes = [(d,), (d,)] + [(d, d), (d,)] * 4 + [(d,), (d,), (d_ff, d), (d_ff,), (d, d_ff), (d,)]
        if not all(p.is_cuda and p.dtype == torch.float32 for p in lt) or [tuple(p.shape) for p in lt] != shapes:
            return False
        if not lib.apq_enc_qkv_ok(*_qkv_args(layer, lt, fresh, fresh, fresh, fresh, b, t, d)):
            return False
        if not lib.apq_enc_attn_ff_ok(*_attn_args(layer, lt, final, fresh, fresh, fresh, fresh, fresh, b, t, d)):
            return False
    return True


def workspace_elements(b, t, d=Q.ENC_D):
    """float32 elements of the q / k / v workspace of a (B, T) batch"""
    return 3 * b * t * d


def encoder_forward(encoder, x, workspace=None):
    """(B, T, in_size) -> (B, T, 64) = ``encoder(x)`` without a mask, on the kernels: two launches per layer.  ``workspace``: a
    contiguous float32 CUDA tensor of at least ``workspace_elements(B, T)`` elements (default: allocated here); q, k and v each start a
    third of it apart (rounded down to 16 bytes), and what lies behind their B T 64 elements is never touched.  The caller has asked ``supported`` first: a shape the library does not serve
    raises."""
    lib = Q.lib()
    b, t, _ = x.shape
    d = encoder.pe.d_model
    emb = encoder.embed.embed
    h = torch.addmm(emb.bias, x.reshape(b * t, -1), emb.weight.t()).view(b, t, d)
    h = torch.add(encoder.pe.pe[:, :t], h, alpha=math.sqrt(d))                      # pe + sqrt(d_model) h, one launch
    n = b * t * d
    if workspace is None:
        workspace = torch.empty(3 * n, dtype=torch.float32, device=x.device)
    elif not (workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= 3 * n):
        raise ValueError('encoder_forward: workspace must be a contiguous float32 CUDA tensor of at least %d elements' % (3 * n))
    third = workspace.numel() // 3 // 4 * 4
    q, k, v = (ctypes.c_void_p(workspace.data_ptr() + 4 * third * i) for i in range(3))
    final = _final(encoder)
    for i, layer in enumerate(encoder.layers):
        lt = _layer_tensors(layer)
        last = final if i == len(encoder.layers) - 1 else None
        out = torch.empty_like(h)
        Q.check(lib.apq_enc_qkv(*_qkv_args(layer, lt, ops._ptr(h), q, k, v, b, t, d), ops._stream()), 'enc_qkv')
        Q.check(lib.apq_enc_attn_ff(*_attn_args(layer, lt, last, ops._ptr(h), q, k, v, ops._ptr(out), b, t, d), ops._stream()), 'enc_attn_ff')
        h = out
    return h
