"""Module1's audio -> landmark networks and the clip driver above them.

What this file holds:

* the reference's two networks, attribute for attribute, so that its checkpoints load with ``strict=True``:
  ``Audio2LandmarkContent`` = ``Audio2landmark_content`` (Module1/src/models/model_audio2landmark.py:28-90; a 3-layer LSTM over
  18-frame mel windows, behind the ``fc_prior`` MLP when ``use_prior_net``, + a 3-layer MLP) and ``Audio2LandmarkPos`` =
  ``Audio2landmark_pos`` (:296-386; LSTM audio encoder, speaker-embedding MLP, a 2-layer / 2-head self-attention encoder, :94-262,
  output MLP; its never-run ``Decoder`` is built too because its tensors are in the checkpoint);
* the clip drivers: ``predict_landmarks_speaker_aware`` = ``Audio2landmark_model.test`` (train_audio2landmark.py:247-338) and
  ``predict_landmarks``, the content branch alone; ``to_image_landmarks``, ``register_face`` and ``stabilise_head``, which send a CUDA
  tensor to ``landmark_post`` (libapseq.so) and everything else to ``landmark_host`` (the reference's numpy / scipy statements);
* ``load_module1`` and the photo's face normalisation.  Training the content branch is module1_train.py.

The four switches (``set_X_backend(name)`` returns the previous name, ``get_X_backend()``; the variable is read at import; an unknown
name is a ``ValueError``).  The first choice is the default, and what the last column names always runs on it:

  X           variable                  choices          never served by the kernels
  lstm        APAMD_MODULE1_LSTM        library | hip    CPU tensors, training mode, autograd (nn.LSTM; hip: lstm_hip.py)
  lstm_train  APAMD_MODULE1_LSTM_TRAIN  library | hip    anything but the content branch in training with gradients
  encoder     APAMD_MODULE1_ENCODER     library | hip    CPU tensors, a mask, training with gradients (hip: encoder_hip.py)
  post        APAMD_MODULE1_POST        host | device    CPU tensors and CPU networks (device: the sequence stays a CUDA tensor)

NOT built: the reference's librosa / pysptk / pyworld / resemblyzer front end; callers pass the (T, 18, 80) mel windows and the
256-d speaker embedding its ``au_data`` / ``au_emb`` hold.
"""
import copy
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import landmark_host, landmark_post

FACE_ID_FEAT_SIZE = 204       # 68 x 3, model_audio2landmark.py:23

LSTM_BACKENDS = ('library', 'hip')
POST_BACKENDS = ('host', 'device')
ENCODER_BACKENDS = ('library', 'hip')


class _Switch:
    """One backend choice: ``what`` names it in messages, ``env`` is read once, here; ``value`` is the current choice."""

    def __init__(self, what, env, choices, default):
        self.what, self.choices = what, choices
        self.value = self.checked(os.environ.get(env) or default)

    def checked(self, name):
        if name not in self.choices:
            raise ValueError('Module1 %s backend %r (known: %s)' % (self.what, name, ', '.join(self.choices)))
        return name

    def set(self, name):
        """Select ``name`` (the module docstring's table says what for); returns the previous choice.  An unknown name raises
        ``ValueError`` and leaves the choice as it was."""
        prev, self.value = self.value, self.checked(name)
        return prev

    def get(self):
        """The current choice."""
        return self.value


_lstm = _Switch('LSTM', 'APAMD_MODULE1_LSTM', LSTM_BACKENDS, 'library')
_lstm_train = _Switch('LSTM', 'APAMD_MODULE1_LSTM_TRAIN', LSTM_BACKENDS, 'library')
_encoder = _Switch('encoder', 'APAMD_MODULE1_ENCODER', ENCODER_BACKENDS, 'library')
_post = _Switch('post-processing', 'APAMD_MODULE1_POST', POST_BACKENDS, 'host')
set_lstm_backend, get_lstm_backend = _lstm.set, _lstm.get
set_lstm_train_backend, get_lstm_train_backend = _lstm_train.set, _lstm_train.get
set_encoder_backend, get_encoder_backend = _encoder.set, _encoder.get
set_post_backend, get_post_backend = _post.set, _post.get


def _lstm_last(lstm, x, trainable=False):
    """``lstm(x)[0][:, -1, :]``, the one thing both networks read from their LSTM.  ``trainable``: the caller takes part in the
    training switch (the content branch)."""
    if trainable and lstm.training and torch.is_grad_enabled():
        if _lstm_train.value == 'hip':
            from . import lstm_hip
            return lstm_hip.lstm_train_batched(lstm, x, last_only=True)
        return lstm(x)[0][:, -1, :]
    if _lstm.value == 'hip':
        from . import lstm_hip
        return lstm_hip.lstm_forward_batched(lstm, x, last_only=True)
    return lstm(x)[0][:, -1, :]


def _mlp3(cin, h1, h2, cout, slope):
    return nn.Sequential(nn.Linear(cin, h1), nn.LeakyReLU(slope), nn.Linear(h1, h2), nn.LeakyReLU(slope), nn.Linear(h2, cout))


class Audio2LandmarkContent(nn.Module):
    def __init__(self, num_window_frames=18, in_size=80, lstm_size=161, use_prior_net=False, hidden_size=256, num_layers=3,
                 drop_out=0.0):
        super().__init__()
        # (the reference assigns fc_prior and fc to the same Sequential first and then replaces fc, :33-38 / :62-70:
        # both exist in its state_dict, registered in the order fc_prior, fc, bilstm)
        self.fc_prior = nn.Sequential(nn.Linear(in_size, 256), nn.BatchNorm1d(256), nn.LeakyReLU(0.2),
                                      nn.Linear(256, lstm_size))
        self.fc = self.fc_prior
        self.use_prior_net = use_prior_net
        self.bilstm = nn.LSTM(input_size=lstm_size if use_prior_net else in_size, hidden_size=hidden_size,
                              num_layers=num_layers, dropout=drop_out, bidirectional=False, batch_first=True)   # :41-55
        self.fc = nn.Sequential(nn.Linear(hidden_size + FACE_ID_FEAT_SIZE, 512), nn.BatchNorm1d(512), nn.LeakyReLU(0.2),
                                nn.Linear(512, 256), nn.BatchNorm1d(256), nn.LeakyReLU(0.2), nn.Linear(256, 204))
        self.in_size, self.lstm_size, self.num_window_frames = in_size, lstm_size, num_window_frames

    def forward(self, au, face_id):                                              # :74-88
        x = au
        if self.use_prior_net:
            x = self.fc_prior(x.contiguous().view(-1, self.in_size)).view(-1, self.num_window_frames, self.lstm_size)
        output = _lstm_last(self.bilstm, x, trainable=True)
        if face_id.shape[0] == 1:
            face_id = face_id.repeat(output.shape[0], 1)
        return self.fc(torch.cat((output, face_id), dim=1)), face_id


# ---------------------------------------------------------------------------------------------- self-attention pieces
class Embedder(nn.Module):                                                       # :94-99
    def __init__(self, feat_size, d_model):
        super().__init__()
        self.embed = nn.Linear(feat_size, d_model)

    def forward(self, x):
        return self.embed(x)


class PositionalEncoder(nn.Module):                                              # :102-127 (its own sin / cos exponents)
    def __init__(self, d_model, max_seq_len=512):
        super().__init__()
        self.d_model = d_model
        pos = torch.arange(max_seq_len, dtype=torch.float64).unsqueeze(1)
        i = torch.arange(0, d_model, 2, dtype=torch.float64).unsqueeze(0)
        pe = torch.zeros(max_seq_len, d_model, dtype=torch.float64)
        pe[:, 0::2] = torch.sin(pos / (10000 ** ((2 * i) / d_model)))
        pe[:, 1::2] = torch.cos(pos / (10000 ** ((2 * (i + 1)) / d_model)))
        self.register_buffer('pe', pe.float().unsqueeze(0))

    def forward(self, x):
        return x * math.sqrt(self.d_model) + self.pe[:, :x.size(1)]


class MultiHeadAttention(nn.Module):                                             # :130-183
    def __init__(self, heads, d_model, dropout=0.1):
        super().__init__()
        self.d_model, self.d_k, self.h = d_model, d_model // heads, heads
        self.q_linear = nn.Linear(d_model, d_model)
        self.v_linear = nn.Linear(d_model, d_model)
        self.k_linear = nn.Linear(d_model, d_model)
        self.dropout = nn.Dropout(dropout)
        self.out = nn.Linear(d_model, d_model)

    def forward(self, q, k, v, mask=None):
        bs = q.size(0)
        k = self.k_linear(k).view(bs, -1, self.h, self.d_k).transpose(1, 2)
        q = self.q_linear(q).view(bs, -1, self.h, self.d_k).transpose(1, 2)
        v = self.v_linear(v).view(bs, -1, self.h, self.d_k).transpose(1, 2)
        scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(self.d_k)
        if mask is not None:
            scores = scores.masked_fill(mask.unsqueeze(1) == 0, -1e9)
        scores = self.dropout(F.softmax(scores, dim=-1))
        return self.out(torch.matmul(scores, v).transpose(1, 2).contiguous().view(bs, -1, self.d_model))


class FeedForward(nn.Module):                                                    # :185-195
    def __init__(self, d_model, d_ff=2048, dropout=0.1):
        super().__init__()
        self.linear_1 = nn.Linear(d_model, d_ff)
        self.dropout = nn.Dropout(dropout)
        self.linear_2 = nn.Linear(d_ff, d_model)

    def forward(self, x):
        return self.linear_2(self.dropout(F.relu(self.linear_1(x))))


class Norm(nn.Module):                                                           # :198-211 (std unbiased, eps on the std)
    def __init__(self, d_model, eps=1e-6):
        super().__init__()
        self.alpha = nn.Parameter(torch.ones(d_model))
        self.bias = nn.Parameter(torch.zeros(d_model))
        self.eps = eps

    def forward(self, x):
        return self.alpha * (x - x.mean(dim=-1, keepdim=True)) / (x.std(dim=-1, keepdim=True) + self.eps) + self.bias


class EncoderLayer(nn.Module):                                                   # :214-229
    def __init__(self, d_model, heads, dropout=0.1):
        super().__init__()
        self.norm_1, self.norm_2 = Norm(d_model), Norm(d_model)
        self.attn = MultiHeadAttention(heads, d_model)
        self.ff = FeedForward(d_model)
        self.dropout_1, self.dropout_2 = nn.Dropout(dropout), nn.Dropout(dropout)

    def forward(self, x, mask):
        x2 = self.norm_1(x)
        x = x + self.dropout_1(self.attn(x2, x2, x2, mask))
        return x + self.dropout_2(self.ff(self.norm_2(x)))


class DecoderLayer(nn.Module):                                                   # :233-255 (constructed, never run)
    def __init__(self, d_model, heads, dropout=0.1):
        super().__init__()
        self.norm_1, self.norm_2, self.norm_3 = Norm(d_model), Norm(d_model), Norm(d_model)
        self.dropout_1, self.dropout_2, self.dropout_3 = nn.Dropout(dropout), nn.Dropout(dropout), nn.Dropout(dropout)
        self.attn_1 = MultiHeadAttention(heads, d_model)
        self.attn_2 = MultiHeadAttention(heads, d_model)
        self.ff = FeedForward(d_model)

    def forward(self, x, e_outputs, src_mask, trg_mask):
        x2 = self.norm_1(x)
        x = x + self.dropout_1(self.attn_1(x2, x2, x2, trg_mask))
        x = x + self.dropout_2(self.attn_2(self.norm_2(x), e_outputs, e_outputs, src_mask))
        return x + self.dropout_3(self.ff(self.norm_3(x)))


class _Stack(nn.Module):                                                         # Encoder / Decoder, :262-293
    def __init__(self, layer, d_model, n, in_size):
        super().__init__()
        self.N = n
        self.embed = Embedder(in_size, d_model)
        self.pe = PositionalEncoder(d_model)
        self.layers = nn.ModuleList([copy.deepcopy(layer) for _ in range(n)])
        self.norm = Norm(d_model)


def _encoder_on_kernels(encoder, x, mask):
    """Does ``Encoder.forward`` take the kernels of libapseq.so?  Only with the 'hip' backend, a CUDA tensor, no mask, gradients
    disabled or the module in eval mode, and shapes the library serves (encoder_hip.supported: its host-only ``_ok`` calls)."""
    if not (_encoder.value == 'hip' and x.is_cuda and mask is None and not (torch.is_grad_enabled() and encoder.training)):
        return False
    from . import encoder_hip
    return encoder_hip.supported(encoder, x)


class Encoder(_Stack):
    def __init__(self, d_model, n, heads, in_size):
        super().__init__(EncoderLayer(d_model, heads), d_model, n, in_size)

    def forward(self, x, mask=None):
        if _encoder_on_kernels(self, x, mask):
            from . import encoder_hip
            return encoder_hip.encoder_forward(self, x)
        x = self.pe(self.embed(x))
        for layer in self.layers:
            x = layer(x, mask)
        return self.norm(x)


class Decoder(_Stack):
    def __init__(self, d_model, n, heads, in_size):
        super().__init__(DecoderLayer(d_model, heads), d_model, n, in_size)

    def forward(self, x, e_outputs, src_mask=None, trg_mask=None):
        x = self.pe(self.embed(x))
        for layer in self.layers:
            x = layer(x, e_outputs, src_mask, trg_mask)
        return self.norm(x)


class Audio2LandmarkPos(nn.Module):
    def __init__(self, audio_feat_size=80, c_enc_hidden_size=256, num_layers=3, drop_out=0.0, spk_feat_size=256,
                 spk_emb_enc_size=128, transformer_d_model=32, N=2, heads=2, z_size=128, audio_dim=256):
        super().__init__()
        self.audio_content_encoder = nn.LSTM(input_size=audio_feat_size, hidden_size=c_enc_hidden_size,
                                             num_layers=num_layers, dropout=drop_out, bidirectional=False, batch_first=True)
        self.use_audio_projection = audio_dim != c_enc_hidden_size
        if self.use_audio_projection:
            self.audio_projection = _mlp3(c_enc_hidden_size, 256, 128, audio_dim, 0.02)
        self.spk_emb_encoder = _mlp3(spk_feat_size, 256, 128, spk_emb_enc_size, 0.02)
        d_model = transformer_d_model * heads
        self.encoder = Encoder(d_model, N, heads, in_size=audio_dim + spk_emb_enc_size + z_size)
        self.decoder = Decoder(d_model, N, heads, in_size=204)
        self.out = _mlp3(d_model + z_size, 512, 256, 204, 0.02)

    def forward(self, au, emb, face_id, fls=None, z=None):                       # :354-386 (add_z_spk=False)
        audio_encode = _lstm_last(self.audio_content_encoder, au)
        if self.use_audio_projection:
            audio_encode = self.audio_projection(audio_encode)
        spk_encode = self.spk_emb_encoder(emb)
        src_feat = torch.cat((audio_encode, spk_encode, z), dim=1).unsqueeze(0)  # the segment's windows = ONE sequence
        e_outputs = torch.cat((self.encoder(src_feat)[0], z), dim=1)
        return self.out(e_outputs), face_id[0:1, :], spk_encode


# ------------------------------------------------------------------------------------------------- clip-level pipeline
def register_face(frame, anchor):
    """train_content.py:176-183 (``--use_reg_as_std``): the frame's 68 points moved by ``icp_t_shape(frame, anchor)``.
    Rows are float32 in and out, float64 between.  Returns (204,) float32; a CUDA tensor goes through libapseq.so."""
    if torch.is_tensor(frame) and frame.is_cuda:
        anchor = torch.as_tensor(anchor, dtype=torch.float32, device=frame.device)
        return landmark_post.rigid_register(frame.float().reshape(1, -1), anchor, register=True).view(-1)
    return landmark_host.register_face(frame, anchor)


def stabilise_head(fl, std, centerize_face=False, no_y_rotation=False):
    """The two head-stabilisation switches of the reference's test pass (train_audio2landmark.py:312-338) on (T, 204) landmarks
    (``landmark_host.stabilise_head`` says what they do).  numpy in, numpy out; a CUDA tensor is served by one launch of
    libapseq.so (landmark_post.rigid_register) and stays on the device.  With both switches off ``fl`` is returned as it is."""
    if not (centerize_face or no_y_rotation):
        return fl
    if torch.is_tensor(fl) and fl.is_cuda:
        std = torch.as_tensor(std, dtype=torch.float32, device=fl.device).reshape(-1)
        return landmark_post.rigid_register(fl.float().reshape(-1, FACE_ID_FEAT_SIZE), std, center=centerize_face,
                                            no_x_rot=no_y_rotation)
    return landmark_host.stabilise_head(fl, std.detach().cpu() if torch.is_tensor(std) else std, centerize_face, no_y_rotation)


@torch.no_grad()
def predict_landmarks_speaker_aware(net_g, net_c, au_windows, spk_emb, face_id, amp_pos=0.5, amp_lip_x=2.0, amp_lip_y=2.0,
                                    segment=512, smooth_win=31, close_mouth_ratio=0.99, centerize_face=False,
                                    no_y_rotation=False):
    """``Audio2landmark_model.test`` (train_audio2landmark.py:247-309 with __train_face_and_pos__ :101-141):
    au_windows (T, 18, 80), spk_emb (256,), face_id (204,) -> (T, 204) landmarks in Module1's normalised frame.
    Per 512-window segment: pose branch G (speaker embedding x 3, z = 0) -> Savitzky-Golay over the segment -> lips
    pulled together -> x amp_pos; content branch C on the first 18 frames -> calibrated; sum + face id; inverted-lip fix; the
    nose-top extrapolation.  Then a (5, 3) Savitzky-Golay over the clip, and behind it ``stabilise_head`` against ``face_id``
    when ``centerize_face`` or ``no_y_rotation`` is set (:312-338; off, as in the reference's readme, nothing more runs).
    With the 'device' post-processing backend and networks on the GPU every step behind the networks is a launch of libapseq.so
    (landmark_post), the result is a (T, 204) CUDA tensor and nothing between the windows and it touches the host; otherwise the
    steps are landmark_host's and the result a numpy array.  A segment of fewer than 10 windows is dropped (:288-289)."""
    net_g.eval()
    net_c.eval()
    dev = next(net_g.parameters()).device
    au = torch.as_tensor(au_windows, dtype=torch.float32, device=dev)
    emb = torch.as_tensor(spk_emb, dtype=torch.float32, device=dev).view(1, -1).expand(au.shape[0], -1)
    fid = torch.as_tensor(face_id, dtype=torch.float32, device=dev).view(1, FACE_ID_FEAT_SIZE)
    on_device = _post.value == 'device' and dev.type == 'cuda'
    post = landmark_post if on_device else landmark_host
    take = (lambda t: t) if on_device else (lambda t: t.cpu().numpy())           # what the post-processing module is handed
    lens = [min(segment, au.shape[0] - j) for j in range(0, au.shape[0], segment)]       # kept segments: known from the shapes
    kept = sum(n for n in lens if n >= 10)
    if kept == 0:
        raise ValueError('predict_landmarks_speaker_aware: no segment of at least 10 windows')
    fl = (torch.empty((kept, FACE_ID_FEAT_SIZE), dtype=torch.float32, device=dev) if on_device
          else np.empty((kept, FACE_ID_FEAT_SIZE), dtype=np.float32))
    fid_p, row = take(fid), 0
    for k, n in enumerate(lens):
        if n < 10:
            continue
        a, e = au[k * segment:k * segment + n], emb[k * segment:k * segment + n]
        z = torch.zeros(n, 128, device=dev)
        dis = post.savgol(take(net_g(a, e * 3.0, fid.repeat(n, 1), None, z)[0]), int(min(n - 1, smooth_win) // 2 * 2 + 1))
        base = post.calib_baseline(take(net_c(a[:, 0:18, :], fid)[0]), amp_lip_x, amp_lip_y)
        post.segment_assemble(dis, base, fid_p, close_mouth_ratio, amp_pos, close=True, lip=True, nose=True, out=fl[row:row + n])
        row += n
    return stabilise_head(post.savgol(fl, 5), fid_p.reshape(-1), centerize_face, no_y_rotation)


def to_image_landmarks(fl, scale=1.0, shift=(0.0, 0.0), eyes=True, smooth=True, rng=np.random):
    """main_end2end_module2.py:262-272 on the (T, 204) output above: flip / scale / shift x and y into image pixels,
    ``add_naive_eye``, the two clip-level Savitzky-Golay filters.  Returns (T, 68, 3): a numpy array, or for a CUDA tensor a
    CUDA tensor made by two launches of libapseq.so (the blink frames are drawn from ``rng`` on the host, as there)."""
    if torch.is_tensor(fl) and fl.is_cuda:
        return landmark_post.to_image_landmarks(fl.float(), scale, shift, eyes, smooth, rng)
    return landmark_host.to_image_landmarks(fl, scale, shift, eyes, smooth, rng)


@torch.no_grad()
def predict_landmarks(net, au_windows, face_id, scale=1.0, shift=(0.0, 0.0), segment=512, smooth=True):
    """Content branch only (``__train_face_wo_pos__``): segments of 512 windows through the content net
    (train_audio2landmark.py:279-296), ``fl = displacement + face_id`` (:298), then main_end2end_module2.py:264-271.
    Returns (T, 68, 2) image-pixel landmarks (x, y): a CUDA tensor with the 'device' post-processing backend and a network on
    the GPU, else a numpy array."""
    net.eval()
    dev = next(net.parameters()).device
    au = torch.as_tensor(au_windows, dtype=torch.float32, device=dev)
    fid = torch.as_tensor(face_id, dtype=torch.float32, device=dev).view(1, FACE_ID_FEAT_SIZE)
    outs = []
    for j in range(0, au.shape[0], segment):
        dis, f = net(au[j:j + segment][:, 0:18, :], fid)
        outs.append(dis + f)
    fl = torch.cat(outs, 0)
    if not (_post.value == 'device' and fl.is_cuda):
        fl = fl.cpu().numpy()
    return to_image_landmarks(fl, scale, shift, eyes=False, smooth=smooth)[:, :, :2]


# ------------------------------------------------------------------------------------------------ clip driver pieces
def load_module1(speaker_ckpt, content_ckpt, device=None):
    """The two checkpoints ``Audio2landmark_model.__init__`` loads (train_audio2landmark.py:55-79):
    ``ckpt_speaker_branch.pth`` -> ``G`` (key 'G', minus the ``comb_mlp`` entries) and ``ckpt_content_branch.pth`` -> ``C``
    (key 'model_g_face_id'); both in eval mode on ``device``.  Returns (net_g, net_c)."""
    net_g = Audio2LandmarkPos(drop_out=0.5)                                          # :55-59
    ck = torch.load(speaker_ckpt, map_location='cpu')
    sd = net_g.state_dict()
    sd.update({k: v for k, v in ck['G'].items() if k.split('.')[0] not in ['comb_mlp']})   # :64-66
    net_g.load_state_dict(sd)
    sd_c = torch.load(content_ckpt, map_location='cpu')['model_g_face_id']
    # :71-73 builds it with the prior net; a checkpoint of module1_train.py trained without one says so by its LSTM's width
    # (161 against the 80 mel bands).  A network whose lstm_size equals its in_size cannot be told apart this way: such a
    # checkpoint is not the reference's and is not served here
    for key in ('bilstm.weight_ih_l0', 'fc_prior.0.weight'):
        if key not in sd_c:
            raise KeyError('load_module1: %s has no %r under model_g_face_id: not a content-branch checkpoint' % (content_ckpt, key))
    width, in_size = sd_c['bilstm.weight_ih_l0'].shape[1], sd_c['fc_prior.0.weight'].shape[1]
    if width not in (in_size, 161):
        raise ValueError('load_module1: %s has an LSTM input width of %d: served are %d (no prior net) and 161 (prior net)'
                         % (content_ckpt, width, in_size))
    prior = width != in_size
    net_c = Audio2LandmarkContent(use_prior_net=prior, drop_out=0.5)
    net_c.load_state_dict(sd_c)                                                      # :76-77
    for n in (net_g, net_c):
        n.eval()
        for q in n.parameters():
            q.requires_grad_(False)
    return (net_g.to(device), net_c.to(device)) if device is not None else (net_g, net_c)


def adjust_and_norm_input_face(shape_3d, std_face_z=None):
    """main_end2end_module2.py:196-204 + util/utils.py:348-359 on the photo's (68, 3) landmarks (pixels): the manual lip /
    eye adjustment, then the normalisation to Module1's frame.  Returns (face_id (68, 3), scale, shift (2,)); ``std_face_z``
    is column z of STD_FACE_LANDMARKS.txt (the reference replaces the detected depth by it x 0.1; zeros when absent)."""
    f = np.array(shape_3d, dtype=np.float64, copy=True).reshape(68, 3)
    f[49:54, 1] += 1.
    f[55:60, 1] -= 1.
    f[[37, 38, 43, 44], 1] -= 2
    f[[40, 41, 46, 47], 1] += 2
    scale = 1.6 / (f[0, 0] - f[16, 0])
    shift = -0.5 * (f[0, 0:2] + f[16, 0:2])
    f[:, 0:2] = (f[:, 0:2] + shift) * scale
    f[:, 2] = 0.0 if std_face_z is None else np.asarray(std_face_z, dtype=np.float64).reshape(68) * 0.1
    f[:, 0:2] = -f[:, 0:2]
    return f, float(scale), shift


def photo_landmarks_in_pixels(face_id, scale, shift):
    """main_end2end_module2.py:311-315 ('save ori'): the normalised face back in image pixels, (68, 2)."""
    f = np.array(face_id, dtype=np.float64, copy=True).reshape(68, 3)
    f[:, 0:2] = -f[:, 0:2] / scale - np.asarray(shift, dtype=np.float64)
    return f[:, :2].astype(np.float32)
