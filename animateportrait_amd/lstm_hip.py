"""nn.LSTM forward (inference) with the recurrence on libapamd.so: per layer and direction ONE library GEMM for the input
projections of all time steps and ONE launch of ``ap_lstm_recurrence`` (csrc/lstm.hip) for the time loop -- instead of a few tiny
library kernels per time step (the AutoVC converter's ~830-frame sequences: ~11 k launches, 0.20 s of host time per 10 s clip).

Same parameters, same gate order, same results as ``nn.LSTM`` (tests/test_module1_gpu.py holds it to the library op on the device).
Falls back to the module itself where the kernel does not apply (CPU tensors, training mode, projections, unsupported sizes).

``lstm_forward_batched`` is the other shape: MANY short sequences of a unidirectional LSTM with 256 hidden units (Module1's two
landmark networks: up to 512 windows of 18 frames).  One ``apq_lstm_layer_fwd`` launch of libapseq.so (csrc/seq/seq_lstm.hip) per
layer, input projection included; no library GEMM, no workspace."""
import ctypes

import torch

from . import _capi as C
from . import _seqapi as Q
from . import ops

_WS = {}


def _workspace(h, dev):
    key = (h, str(dev))
    ws = _WS.get(key)
    if ws is None:
        n = int(C.lib().ap_lstm_workspace_bytes(h))
        ws = _WS[key] = torch.zeros(n, dtype=torch.uint8, device=dev)
    return ws


def supported(lstm, x):
    h = lstm.hidden_size
    return (isinstance(lstm, torch.nn.LSTM) and x.is_cuda and x.dtype == torch.float32 and not lstm.training and lstm.batch_first and
            lstm.bias and getattr(lstm, 'proj_size', 0) == 0 and x.dim() == 3 and not torch.is_grad_enabled() and
            (h <= 64 or (h in (256, 512) and x.shape[0] == 1)))


def lstm_forward(lstm, x):
    """(B, T, I) -> (B, T, D * H): ``lstm(x)[0]`` with zero initial state."""
    if not supported(lstm, x):
        return lstm(x)[0]
    lib = C.lib()
    b, t, _ = x.shape
    h, nd = lstm.hidden_size, 2 if lstm.bidirectional else 1
    inp = x.contiguous()
    for layer in range(lstm.num_layers):
        out = torch.empty((b, t, nd * h), dtype=torch.float32, device=x.device)
        for d in range(nd):
            sfx = '_l%d%s' % (layer, '_reverse' if d else '')
            w_ih, w_hh = getattr(lstm, 'weight_ih' + sfx), getattr(lstm, 'weight_hh' + sfx)
            bias = getattr(lstm, 'bias_ih' + sfx) + getattr(lstm, 'bias_hh' + sfx)
            xproj = torch.addmm(bias, inp.reshape(b * t, -1), w_ih.t())              # (B T, 4H): every time step in one GEMM
            ws = _workspace(h, x.device) if h > 64 else None
            C.check(lib.ap_lstm_recurrence(ops._ptr(xproj), ops._ptr(w_hh.contiguous()), None, None, ops._ptr(out), None, None, b, t, h, d,
                                           nd * h, d * h, ops._ptr(ws) if ws is not None else None, ops._stream()), 'lstm_recurrence')
        inp = out
    return inp


def _layer_params(lstm, layer):
    sfx = '_l%d' % layer
    return [getattr(lstm, n + sfx).contiguous() for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]


def supported_batched(lstm, x):
    """The conditions of ``supported`` with 256 hidden units, any batch, one direction -- and the library's own word on the sizes
    and pointers of every layer (apq_lstm_layer_fwd_ok: host only)."""
    if not (isinstance(lstm, torch.nn.LSTM) and x.is_cuda and x.dtype == torch.float32 and not lstm.training and lstm.batch_first and
            lstm.bias and getattr(lstm, 'proj_size', 0) == 0 and x.dim() == 3 and not torch.is_grad_enabled() and
            not lstm.bidirectional and lstm.hidden_size == Q.LSTM_H and x.shape[0] >= 1 and x.shape[1] >= 1):
        return False
    b, t, i = x.shape
    if i != lstm.input_size:
        return False
    lib = Q.lib()
    # lstm_forward_batched allocates every layer's output (and a contiguous copy of a strided x) itself: torch's allocations are
    # aligned far beyond what the kernel asks, so an aligned stand-in address speaks for them
    fresh = ctypes.c_void_p(Q.ALIGN_WIDE)
    for layer in range(lstm.num_layers):
        w_ih, w_hh, b_ih, b_hh = _layer_params(lstm, layer)
        xin = ops._ptr(x) if layer == 0 and x.is_contiguous() else fresh
        if not lib.apq_lstm_layer_fwd_ok(xin, ops._ptr(w_ih), ops._ptr(w_hh), ops._ptr(b_ih), ops._ptr(b_hh), fresh, b, t,
                                         i if layer == 0 else Q.LSTM_H, Q.LSTM_H, 0):
            return False
    return True


def lstm_forward_batched(lstm, x, last_only=False):
    """(B, T, I) -> (B, T, H) = ``lstm(x)[0]`` with zero initial state, or with ``last_only`` (B, H) = ``lstm(x)[0][:, -1, :]``:
    one apq_lstm_layer_fwd launch per layer.  Falls back to the module where ``supported_batched`` says no."""
    if not supported_batched(lstm, x):
        out = lstm(x)[0]
        return out[:, -1, :] if last_only else out
    lib = Q.lib()
    b, t, _ = x.shape
    h = lstm.hidden_size
    inp = x.contiguous()
    for layer in range(lstm.num_layers):
        last = last_only and layer == lstm.num_layers - 1
        out = torch.empty((b, h) if last else (b, t, h), dtype=torch.float32, device=x.device)
        w_ih, w_hh, b_ih, b_hh = _layer_params(lstm, layer)
        Q.check(lib.apq_lstm_layer_fwd(ops._ptr(inp), ops._ptr(w_ih), ops._ptr(w_hh), ops._ptr(b_ih), ops._ptr(b_hh), ops._ptr(out),
                                       b, t, inp.shape[2], h, 1 if last else 0, ops._stream()), 'lstm_layer_fwd')
        inp = out
    return inp


def check_timeouts():
    """After a synchronisation: did a distributed launch give up waiting for its peer workgroups (a device shared with other work)?"""
    for (h, _), ws in _WS.items():
        if C.lib().ap_lstm_timed_out(ctypes.c_void_p(ws.data_ptr()), h) == 1:
            raise RuntimeError('ap_lstm_recurrence (H = %d): the workgroups of a launch never met; its output is invalid' % h)
