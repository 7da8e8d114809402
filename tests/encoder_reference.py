"""The pose network's self-attention encoder restated in float64 numpy (own code, written from ``module1.Encoder`` and the
reference's ``Encoder``, Module1/src/models/model_audio2landmark_speaker_aware.py:195-209 with the pieces at :26-161): the contract
of animateportrait_amd/encoder_hip.py and csrc/seq/seq_encoder.hip, and the reference of their tests.

    h = embed(x) sqrt(d_model) + pe[:T]
    per layer:  n = Norm_1(h);  q, k, v = the three projections of n, split into heads of d_k columns (head-major);
                c = the heads' softmax(q k^T / sqrt(d_k)) v side by side;  h = h + out(c);  h = h + linear_2(relu(linear_1(Norm_2(h))))
    Norm(h)

``Norm`` is alpha (x - mean) / (std + eps) + bias with the UNBIASED standard deviation and eps added to the std.  No mask, no
dropout (inference).  ``params`` is the module's state_dict as float64 numpy arrays (``params_of``)."""
import numpy as np


def params_of(encoder):
    """state_dict of a ``module1.Encoder`` -> {name: float64 array}"""
    return {k: v.detach().cpu().double().numpy() for k, v in encoder.state_dict().items()}


def norm(x, alpha, bias, eps=1e-6):
    mean = x.mean(axis=-1, keepdims=True)
    std = np.sqrt(((x - mean) ** 2).sum(axis=-1, keepdims=True) / (x.shape[-1] - 1))
    return alpha * (x - mean) / (std + eps) + bias


def linear(x, w, b):
    return x @ w.T + b


def attention_scores(n, p, pre, heads):
    """(B, heads, T, T): q k^T / sqrt(d_k) of layer ``pre`` on its normalised input n (B, T, d_model), before the softmax"""
    b, t, d = n.shape
    dk = d // heads
    q = linear(n, p[pre + 'attn.q_linear.weight'], p[pre + 'attn.q_linear.bias']).reshape(b, t, heads, dk).transpose(0, 2, 1, 3)
    k = linear(n, p[pre + 'attn.k_linear.weight'], p[pre + 'attn.k_linear.bias']).reshape(b, t, heads, dk).transpose(0, 2, 1, 3)
    return q @ k.transpose(0, 1, 3, 2) / np.sqrt(dk)


def encoder_layer(h, p, pre, heads, eps=1e-6):
    b, t, d = h.shape
    dk = d // heads
    n = norm(h, p[pre + 'norm_1.alpha'], p[pre + 'norm_1.bias'], eps)
    s = attention_scores(n, p, pre, heads)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    prob = e / e.sum(axis=-1, keepdims=True)
    v = linear(n, p[pre + 'attn.v_linear.weight'], p[pre + 'attn.v_linear.bias']).reshape(b, t, heads, dk).transpose(0, 2, 1, 3)
    c = (prob @ v).transpose(0, 2, 1, 3).reshape(b, t, d)
    h = h + linear(c, p[pre + 'attn.out.weight'], p[pre + 'attn.out.bias'])
    n2 = norm(h, p[pre + 'norm_2.alpha'], p[pre + 'norm_2.bias'], eps)
    ff = linear(np.maximum(linear(n2, p[pre + 'ff.linear_1.weight'], p[pre + 'ff.linear_1.bias']), 0.0),
                p[pre + 'ff.linear_2.weight'], p[pre + 'ff.linear_2.bias'])
    return h + ff


def embed(x, p):
    """embed(x) sqrt(d_model) + pe[:T]: the input of layer 0"""
    x = np.asarray(x, dtype=np.float64)
    d = p['embed.embed.weight'].shape[0]
    return linear(x, p['embed.embed.weight'], p['embed.embed.bias']) * np.sqrt(d) + p['pe.pe'][:, :x.shape[1]]


def encoder_forward(x, p, heads=2, eps=1e-6):
    """x (B, T, in_size) -> (B, T, d_model) in float64"""
    h = embed(x, p)
    n_layers = 1 + max(int(k.split('.')[1]) for k in p if k.startswith('layers.'))
    for i in range(n_layers):
        h = encoder_layer(h, p, 'layers.%d.' % i, heads, eps)
    return norm(h, p['norm.alpha'], p['norm.bias'], eps)
