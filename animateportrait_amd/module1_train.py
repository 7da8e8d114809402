"""Train Module1's content branch (the audio -> lip-motion network a user fine-tunes for a new language or speaker): the
counterpart of Module1/src/approaches/train_content.py and its dataset, Module1/src/dataset/audio2landmark/audio2landmark_dataset.py.

    python -m animateportrait_amd.module1_train --dump_dir D --ckpt_dir C --nepoch N [--load_a2l_C_name CKPT] [--lstm library|hip]

* ``ContentDataset`` reads ``<dump_dir>/<dump_name>_{train,test}_{au,fl}.pickle``: each a list of ``(array (T, 80 | 204), info)``,
  the layout main_end2end_module2.py:230-251 writes, clips shuffled with seed 0 as the reference does (:40-45); ``windows`` is
  ``my_collate_in_segments_noemb`` (:86-104).  The mel features are normalised (:47-53) only when ``--au_mean_std FILE`` names
  the reference's table of means and standard deviations: this project's clip front end (audio.py) feeds the networks unnormalised
  features, and a network is trained on what it will be run on.
* ``ContentTrainer`` mirrors train_content.py:80-128 (the loss) and :161-208 (the pass over the clips): the closed-lip identity
  frame picked from every tenth frame, the random start in training, segments of 512 windows (under 10: skipped), the L1 term
  with or without the lip-region weights, the optional motion term, the Laplacian term, ``Adam(lr, weight_decay=reg_lr)``, an
  eval pass under ``no_grad``.  Checkpoints are the reference's: ``{'model_g_face_id': state_dict, 'epoch': N}`` in
  ``ckpt_last_epoch.pth`` and ``ckpt_e_<N>.pth``, which ``module1.load_module1`` and ``end2end.py --load_a2l_C_name`` load.
* ``--lstm hip`` trains the 3-layer LSTM on libapseq.so's kernel pair: ``main`` sets ``module1.set_lstm_train_backend`` for the run and
  restores it; ``ContentTrainer`` itself leaves the switch to its caller.

* ``--use_reg_as_std --std_face FILE`` registers every clip's identity frame onto the standard face before it is used
  (:176-183; ``module1.register_face`` on the host, one frame per clip): FILE is the reference's STD_FACE_LANDMARKS.txt, 68 rows
  "x y z".  The flag without a standard face is refused by name: there is nothing to register onto.

NOT built: the ``Vis`` animation dumps (:226-251) do not exist.  The reference's launcher for this class is not in its tree; DESIGN.md 4e-5 says where the defaults
below come from."""
import argparse
import os
import pickle
import random
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import module1
from .audio import load_mean_std

SEG_BS = 512          # windows of a segment (train_content.py:168)
MIN_SEG = 10          # shorter segments are skipped (:204)

# the Laplacian term's neighbours along the 68-point contours (:112-117)
N1 = ([1] + list(range(0, 16)) + [18] + list(range(17, 21)) + [23] + list(range(22, 26)) + [28] + list(range(27, 35)) + [41] +
      list(range(36, 41)) + [47] + list(range(42, 47)) + [59] + list(range(48, 59)) + [67] + list(range(60, 67)))
N2 = (list(range(1, 17)) + [15] + list(range(18, 22)) + [20] + list(range(23, 27)) + [25] + list(range(28, 36)) + [34] +
      list(range(37, 42)) + [36] + list(range(43, 48)) + [42] + list(range(49, 60)) + [48] + list(range(61, 68)) + [60])


def window_starts(n_frames, num_window_frames, num_window_step):
    """First frame of every window of a clip: range(0, T - W, step) -- the reference's bound, which drops the last full window"""
    return list(range(0, n_frames - num_window_frames, num_window_step))


class ContentDataset:
    def __init__(self, dump_dir, dump_name='autovc_retrain_mel', status='train', num_window_frames=18, num_window_step=1,
                 au_mean_std=None):
        self.num_window_frames, self.num_window_step = num_window_frames, num_window_step
        data = {}
        for kind in ('au', 'fl'):
            path = os.path.join(dump_dir, '%s_%s_%s.pickle' % (dump_name, status, kind))
            with open(path, 'rb') as fp:
                data[kind] = pickle.load(fp)
        if len(data['au']) != len(data['fl']):
            raise ValueError('%s: %d au clips, %d fl clips' % (dump_dir, len(data['au']), len(data['fl'])))
        idx = list(range(len(data['au'])))
        random.Random(0).shuffle(idx)                                            # random.seed(0); random.shuffle(valid_idx)
        self.fl_data = [data['fl'][i] for i in idx]
        self.au_data = [data['au'][i] for i in idx]
        if au_mean_std is not None:
            mean, std = load_mean_std(au_mean_std)
            self.au_data = [((au - mean) / std,) + tuple(rest) for au, *rest in self.au_data]

    def __len__(self):
        return len(self.fl_data)

    def __getitem__(self, item):
        return self.fl_data[item], self.au_data[item]

    def windows(self, item, dtype=torch.float32):
        """(fls (N, W, 204), aus (N, W, 80)) of clip ``item``"""
        fl, au = torch.as_tensor(np.asarray(self.fl_data[item][0]), dtype=dtype), torch.as_tensor(np.asarray(self.au_data[item][0]), dtype=dtype)
        if fl.shape[0] != au.shape[0]:
            raise ValueError('clip %d: %d landmark frames, %d audio frames' % (item, fl.shape[0], au.shape[0]))
        w = self.num_window_frames
        starts = window_starts(fl.shape[0], w, self.num_window_step)
        if not starts:
            return fl.new_zeros((0, w, fl.shape[1])), au.new_zeros((0, w, au.shape[1]))
        return torch.stack([fl[i:i + w] for i in starts]), torch.stack([au[i:i + w] for i in starts])


def close_face_lip(fl):
    """__close_face_lip__ (:274-283) on (N, 204): the frame whose inner-lip polygon (points 60..67) has the smallest area, the
    area as the reference sums it: unsigned triangles of the fan from the first vertex."""
    pts = np.asarray(fl, dtype=np.float64).reshape(-1, 68, 3)[:, 60:68, 0:2]
    ab, ac = pts[:, 1:-1] - pts[:, 0:1], pts[:, 2:] - pts[:, 0:1]
    area = 0.5 * np.abs(ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0])
    best, idx = 999, 0
    for i in range(area.shape[0]):
        s = 0
        for tri in area[i]:
            s += tri
        if s < best:
            best, idx = s, i
    return idx


def content_loss(net, fls, aus, face_id, use_lip_weight=True, use_motion_loss=False, lambda_laplacian_smooth_loss=1.0):
    """The loss of __train_content__ (:80-123) for one segment: fls (N, W, 204), aus (N, W, 80), face_id (1 | N, 204).
    Returns (loss, fl_dis_pred (N, 204))."""
    fls_gt = fls[:, 0, :].detach().clone()
    if face_id.shape[0] == 1:
        face_id = face_id.repeat(aus.shape[0], 1)
    fl_dis_pred, _ = net(aus, face_id)
    w = torch.abs(fls[:, 0, 66 * 3 + 1] - fls[:, 0, 62 * 3 + 1])
    # (both constants are float32 whatever fls is, as in the reference: in a float64 run the weights are float32 values)
    w = torch.tensor([1.0], device=fls.device) / (w * 4.0 + 0.1)
    lip_region_w = torch.ones((fls.shape[0], 204), device=fls.device)
    lip_region_w[:, 48 * 3:] = torch.cat([w.unsqueeze(1)] * 60, dim=1)
    lip_region_w = lip_region_w.detach()
    pred = fl_dis_pred + face_id[0:1].detach()
    if use_lip_weight:
        loss = torch.mean(torch.abs(pred - fls_gt) * lip_region_w)
    else:
        loss = F.l1_loss(pred, fls_gt)
    if use_motion_loss:
        loss = loss + F.l1_loss(fl_dis_pred[:-1] - fl_dis_pred[1:], fls_gt[:-1] - fls_gt[1:])
    if lambda_laplacian_smooth_loss > 0.0:                                          # (a switch, not a factor: :111, :123)
        v = pred.view(-1, 68, 3)
        l_v = v - 0.5 * (v[:, N1, :] + v[:, N2, :])
        gt = fls_gt.view(-1, 68, 3)
        l_g = gt - 0.5 * (gt[:, N1, :] + gt[:, N2, :])
        loss = loss + F.l1_loss(l_v, l_g)
    return loss, fl_dis_pred


def load_std_face(path):
    """STD_FACE_LANDMARKS.txt: 68 rows "x y z" -> (204,) float32, the anchor of ``--use_reg_as_std``"""
    std = np.loadtxt(path, dtype=np.float64)
    if std.size != 204:
        raise ValueError('%s: %d numbers, a standard face has 68 x 3' % (path, std.size))
    return std.reshape(204).astype(np.float32)


class ContentTrainer:
    def __init__(self, opt, device=None, dtype=torch.float32):
        self.anchor = None
        if getattr(opt, 'use_reg_as_std', False):
            if not getattr(opt, 'std_face', None):
                raise NotImplementedError('--use_reg_as_std without --std_face: the registration of the identity frame needs the '
                                          'standard face to register onto')
            self.anchor = load_std_face(opt.std_face)
        self.opt = opt
        self.device = torch.device(device if device is not None else ('cuda:0' if torch.cuda.is_available() else 'cpu'))
        self.dtype = dtype
        kw = dict(dump_dir=opt.dump_dir, dump_name=opt.dump_name, num_window_frames=opt.num_window_frames,
                  num_window_step=opt.num_window_step, au_mean_std=getattr(opt, 'au_mean_std', None))
        self.train_data = ContentDataset(status='train', **kw)
        self.eval_data = ContentDataset(status='test', **kw)
        self.C = module1.Audio2LandmarkContent(num_window_frames=opt.num_window_frames, hidden_size=opt.hidden_size, in_size=opt.in_size,
                                               use_prior_net=bool(opt.use_prior_net), drop_out=opt.drop_out)
        if opt.load_a2l_C_name and os.path.basename(opt.load_a2l_C_name) != '':
            self.C.load_state_dict(torch.load(opt.load_a2l_C_name, map_location='cpu')['model_g_face_id'])
        self.C.to(device=self.device, dtype=dtype)
        self.opt_C = torch.optim.Adam(self.C.parameters(), lr=opt.lr, weight_decay=opt.reg_lr)
        self.rng = np.random.RandomState(getattr(opt, 'seed', None))

    def train_content(self, fls, aus, face_id, is_training=True):
        """__train_content__: the loss of one segment and, in training, one Adam step.  Returns (fl_dis_pred, loss)."""
        o = self.opt
        loss, pred = content_loss(self.C, fls, aus, face_id, bool(o.use_lip_weight), bool(o.use_motion_loss),
                                  o.lambda_laplacian_smooth_loss)
        if is_training:
            self.opt_C.zero_grad()
            loss.backward()
            self.opt_C.step()
        return pred.detach(), loss.detach()

    def run_pass(self, epoch, is_training=True):
        """__train_pass__ (:142-208, :269-271) without the animation dumps.  Returns the mean loss over the segments."""
        self.C.train(is_training)
        data = self.train_data if is_training else self.eval_data
        losses = []
        t0 = time.time()
        with torch.set_grad_enabled(is_training):
            for i in range(len(data)):
                fl_ori, au_ori = (a.to(self.device) for a in data.windows(i, self.dtype))
                if fl_ori.shape[0] == 0:
                    continue
                close_fl = fl_ori[::10, 0, :]                                        # :171-173
                idx = close_face_lip(close_fl.detach().cpu().numpy())
                face_id = close_fl[idx:idx + 1, :]
                if self.anchor is not None:                                          # :176-183
                    face_id = self.registered_face_id(face_id)
                for _ in range(self.opt.in_batch_nepoch):
                    start = 0
                    if is_training:                                                  # :189-192
                        start = int(self.rng.randint(0, max(fl_ori.shape[0] // 5, 1), 1).reshape(-1)[0])
                    fl, au = fl_ori[start:], au_ori[start:]
                    for j in range(0, fl.shape[0], SEG_BS):
                        fl_seg, au_seg = fl[j:j + SEG_BS], au[j:j + SEG_BS]
                        if fl_seg.shape[0] < MIN_SEG:
                            continue
                        _, loss = self.train_content(fl_seg, au_seg, face_id, is_training)
                        losses.append(float(loss))
        mean = float(np.mean(losses)) if losses else float('nan')
        print('%s Epoch: #%d loss %.5f (%d segments, %.2f sec)' % ('TRAIN' if is_training else 'EVAL', epoch, mean, len(losses),
                                                                  time.time() - t0))
        if is_training:
            self.save('last_epoch', epoch)
            if epoch % self.opt.ckpt_epoch_freq == 0:
                self.save('e_%d' % epoch, epoch)
        return mean

    def registered_face_id(self, face_id):
        """The (1, 204) identity frame registered onto the standard face: through float32 on the host, as the reference does."""
        reg = module1.register_face(face_id.detach().cpu().numpy().astype(np.float32), self.anchor)
        return torch.as_tensor(reg.reshape(1, 204), dtype=self.dtype, device=self.device)

    def save(self, save_type, epoch):
        os.makedirs(self.opt.ckpt_dir, exist_ok=True)
        sd = {k: v.detach().cpu() for k, v in self.C.state_dict().items()}
        torch.save({'model_g_face_id': sd, 'epoch': epoch}, os.path.join(self.opt.ckpt_dir, 'ckpt_%s.pth' % save_type))

    def train(self):
        out = []
        for epoch in range(self.opt.nepoch):
            out.append((self.run_pass(epoch, True), self.run_pass(epoch, False)))
        return out


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dump_dir', required=True)
    ap.add_argument('--dump_name', default='autovc_retrain_mel')
    ap.add_argument('--ckpt_dir', required=True)
    ap.add_argument('--nepoch', type=int, required=True)
    ap.add_argument('--load_a2l_C_name', default='')
    ap.add_argument('--lstm', choices=module1.LSTM_BACKENDS, default=None, help='who trains the LSTM (default: APAMD_MODULE1_LSTM_TRAIN, else library)')
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--reg_lr', type=float, default=1e-6, help='Adam weight decay')
    ap.add_argument('--use_lip_weight', type=int, default=1)
    ap.add_argument('--use_motion_loss', type=int, default=0)
    ap.add_argument('--lambda_laplacian_smooth_loss', type=float, default=1.0)
    ap.add_argument('--in_batch_nepoch', type=int, default=1)
    ap.add_argument('--num_window_frames', type=int, default=18)
    ap.add_argument('--num_window_step', type=int, default=1)
    ap.add_argument('--hidden_size', type=int, default=256)
    ap.add_argument('--in_size', type=int, default=80)
    ap.add_argument('--drop_out', type=float, default=0.0)
    ap.add_argument('--use_prior_net', type=int, default=0)
    ap.add_argument('--ckpt_epoch_freq', type=int, default=1)
    ap.add_argument('--use_reg_as_std', action='store_true',
                    help='register every clip\'s identity frame onto the standard face (train_content.py:176-183); needs --std_face')
    ap.add_argument('--std_face', default=None, help='STD_FACE_LANDMARKS.txt, 68 rows "x y z": the anchor of --use_reg_as_std')
    ap.add_argument('--au_mean_std', default=None, help='table of mel means and standard deviations to normalise with (default: none)')
    ap.add_argument('--seed', type=int, default=None, help='seed of the random segment starts')
    ap.add_argument('--device', default=None)
    return ap


def main(argv=None):
    opt = make_parser().parse_args(argv)
    if opt.use_reg_as_std and not opt.std_face:
        raise SystemExit('module1_train: --use_reg_as_std is refused without --std_face: the registration of the identity frame '
                         'needs the standard face to register onto')
    # the switch is the process's: set for this run, put back behind it (a caller of ContentTrainer sets it itself)
    prev = module1.set_lstm_train_backend(opt.lstm) if opt.lstm else None
    try:
        ContentTrainer(opt, device=opt.device).train()
    finally:
        if prev is not None:
            module1.set_lstm_train_backend(prev)
    return 0


if __name__ == '__main__':
    sys.exit(main())
