"""nn.LSTM forward (inference) with the recurrence on libapamd.so: per layer and direction ONE library GEMM for the input
projections of all time steps and ONE launch of ``ap_lstm_recurrence`` (csrc/lstm.hip) for the time loop -- instead of a few tiny
library kernels per time step (the AutoVC converter's ~830-frame sequences: ~11 k launches, 0.20 s of host time per 10 s clip).

Same parameters, same gate order, same results as ``nn.LSTM`` (tests/test_module1_gpu.py holds it to the library op on the device).
Falls back to the module itself where the kernel does not apply (CPU tensors, training mode, projections, unsupported sizes).

``lstm_forward_batched`` is the other shape: MANY short sequences of a unidirectional LSTM with 256 hidden units (Module1's two
landmark networks: up to 512 windows of 18 frames).  One ``apq_lstm_layer_fwd`` launch of libapseq.so (csrc/seq/seq_lstm.hip) per
layer, input projection included; no library GEMM, no workspace.

``lstm_train_batched`` is that shape with gradients (training Module1's content branch, module1_train.py): an autograd function
with one ``apq_lstm_layer_fwd_train`` / ``apq_lstm_layer_bwd`` launch pair per layer (csrc/seq/seq_lstm_train.hip)."""
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


def supported_train_batched(lstm, x):
    """What ``lstm_train_batched`` serves: nn.LSTM with batch_first, bias, one direction, no projection, no dropout, 256 hidden
    units, on CUDA fp32 -- and the library's own word on every layer (apq_lstm_layer_fwd_train_ok / apq_lstm_layer_bwd_ok: host
    only).  Training mode and enabled gradients are the caller's business: the path is correct without them, only wasteful."""
    if not (isinstance(lstm, torch.nn.LSTM) and x.is_cuda and x.dtype == torch.float32 and lstm.batch_first and lstm.bias and
            getattr(lstm, 'proj_size', 0) == 0 and lstm.dropout == 0 and x.dim() == 3 and not lstm.bidirectional and
            lstm.hidden_size == Q.LSTM_H and x.shape[0] >= 1 and x.shape[1] >= 1 and x.shape[2] == lstm.input_size):
        return False
    b, t, i = x.shape
    lib = Q.lib()
    fresh = ctypes.c_void_p(Q.ALIGN_WIDE)            # stands for the tensors lstm_train_batched allocates itself
    for layer in range(lstm.num_layers):
        w_ih, w_hh, b_ih, b_hh = _layer_params(lstm, layer)
        xin = ops._ptr(x) if layer == 0 and x.is_contiguous() else fresh
        if not lib.apq_lstm_layer_fwd_train_ok(xin, ops._ptr(w_ih), ops._ptr(w_hh), ops._ptr(b_ih), ops._ptr(b_hh), fresh, fresh, fresh,
                                               b, t, i if layer == 0 else Q.LSTM_H, Q.LSTM_H):
            return False
        if not lib.apq_lstm_layer_bwd_ok(fresh, fresh, fresh, fresh, fresh, b, t, Q.LSTM_H, 0):
            return False
    return True


class _LstmTrainBatched(torch.autograd.Function):
    """The whole stack: one apq_lstm_layer_fwd_train launch per layer forward, one apq_lstm_layer_bwd launch per layer backward
    (csrc/seq/seq_lstm_train.hip).  Saved between the two: per layer its input, its output, the activated gates and c_t.  The
    time-parallel products of the backward (dx, dW_ih, dW_hh, the bias sums) are fp32 library GEMMs over the B T rows of dG."""

    @staticmethod
    def forward(ctx, x, last_only, *weights):
        lib = Q.lib()
        b, t, _ = x.shape
        h = Q.LSTM_H
        inp = x.contiguous()
        saved = []
        for layer in range(len(weights) // 4):
            w_ih, w_hh, b_ih, b_hh = (w.contiguous() for w in weights[4 * layer:4 * layer + 4])
            out = torch.empty((b, t, h), dtype=torch.float32, device=x.device)
            gates = torch.empty((b, t, 4 * h), dtype=torch.float32, device=x.device)
            cell = torch.empty((b, t, h), dtype=torch.float32, device=x.device)
            Q.check(lib.apq_lstm_layer_fwd_train(ops._ptr(inp), ops._ptr(w_ih), ops._ptr(w_hh), ops._ptr(b_ih), ops._ptr(b_hh),
                                                 ops._ptr(out), ops._ptr(gates), ops._ptr(cell), b, t, inp.shape[2], h, ops._stream()),
                    'lstm_layer_fwd_train')
            saved += [inp, out, gates, cell]
            inp = out
        ctx.save_for_backward(*saved, *weights)
        ctx.last_only, ctx.layers = bool(last_only), len(weights) // 4
        return inp[:, -1, :].clone() if last_only else inp

    @staticmethod
    @torch.autograd.function.once_differentiable          # (a second backward through the kernels is an error, not a silent zero)
    def backward(ctx, dout):
        lib = Q.lib()
        n = ctx.layers
        saved, weights = ctx.saved_tensors[:4 * n], ctx.saved_tensors[4 * n:]
        h = Q.LSTM_H
        dout = dout.contiguous()
        last = ctx.last_only
        grads = [None] * (4 * n)
        dx = None
        for layer in range(n - 1, -1, -1):
            inp, out, gates, cell = saved[4 * layer:4 * layer + 4]
            w_ih, w_hh = weights[4 * layer], weights[4 * layer + 1]
            b, t, i = inp.shape
            w_hh_t = w_hh.t().contiguous()                                          # (H, 4H): a lane's four K values are 16 bytes
            dg = torch.empty((b, t, 4 * h), dtype=torch.float32, device=inp.device)
            Q.check(lib.apq_lstm_layer_bwd(ops._ptr(dout), ops._ptr(gates), ops._ptr(cell), ops._ptr(w_hh_t), ops._ptr(dg), b, t, h,
                                           1 if last else 0, ops._stream()), 'lstm_layer_bwd')
            dg2 = dg.view(b * t, 4 * h)
            needs = ctx.needs_input_grad[2 + 4 * layer:6 + 4 * layer]
            if needs[0]:
                grads[4 * layer] = torch.matmul(dg2.t(), inp.reshape(b * t, i))
            if needs[1]:
                h_prev = torch.zeros_like(out)                                       # h_{t-1}, zero initial state
                h_prev[:, 1:] = out[:, :-1]
                grads[4 * layer + 1] = torch.matmul(dg2.t(), h_prev.view(b * t, h))
            if needs[2] or needs[3]:
                db = dg2.sum(0)
                grads[4 * layer + 2] = db if needs[2] else None
                grads[4 * layer + 3] = db.clone() if needs[3] else None
            if layer > 0 or ctx.needs_input_grad[0]:
                dx = torch.matmul(dg2, w_ih).view(b, t, i)
            dout, last = dx, False
        return (dx if ctx.needs_input_grad[0] else None, None, *grads)


def lstm_train_batched(lstm, x, last_only=False):
    """``lstm(x)[0]`` (or with ``last_only`` ``lstm(x)[0][:, -1, :]``) with zero initial state, differentiable in x and in the
    module's parameters, on the training kernel pair of libapseq.so.  Falls back to the module where
    ``supported_train_batched`` says no."""
    if not supported_train_batched(lstm, x):
        out = lstm(x)[0]
        return out[:, -1, :] if last_only else out
    weights = [getattr(lstm, n + '_l%d' % layer) for layer in range(lstm.num_layers)
               for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    return _LstmTrainBatched.apply(x, bool(last_only), *weights)


def check_timeouts():
    """After a synchronisation: did a distributed launch give up waiting for its peer workgroups (a device shared with other work)?"""
    for (h, _), ws in _WS.items():
        if C.lib().ap_lstm_timed_out(ctypes.c_void_p(ws.data_ptr()), h) == 1:
            raise RuntimeError('ap_lstm_recurrence (H = %d): the workgroups of a launch never met; its output is invalid' % h)
