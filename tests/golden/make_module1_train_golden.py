#!/usr/bin/env python3
"""Golden for training Module1's content branch (tests/golden/module1_train.npz): the reference's ``Audio2landmark_content``
(Module1/src/models/model_audio2landmark.py:28-90) in training mode and the loss of ``Audio2landmark_model.__train_content__``
(Module1/src/approaches/train_content.py:80-140), called on a namespace that carries what it reads, in float64 on the CPU: one
40-window segment, seeded weights (``make_module1_golden.seeded_state``, seed 81, use_prior_net=True so that every tensor of
the network gets a gradient), all four combinations of the lip weights and the motion term.  Per combination: the loss, and
per parameter tensor the L2 norm and 64 sampled entries (``sample_index``) of its gradient and of its value after the one Adam
step the method takes (lr 1e-3, weight_decay 1e-6).  Also the window indices ``my_collate_in_segments_noemb``
(Module1/src/dataset/audio2landmark/audio2landmark_dataset.py:86-104) makes of a 60-frame clip.  Samples, not whole tensors:
the file stays small.
Shims: an empty ``cv2`` module; the approach module's ``device`` set to the CPU.
Run in the build container:  python tests/golden/make_module1_train_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

SEED, N_WIN, N_SAMPLES = 81, 40, 64
COMBOS = [(lip, motion) for lip in (0, 1) for motion in (0, 1)]       # (use_lip_weight, use_motion_loss)


def sample_index(n):
    """the flat indices of a tensor of n elements the golden keeps: 64 of them, evenly spread, first and last included"""
    return np.linspace(0, n - 1, N_SAMPLES).astype(np.int64)


def segment_inputs():
    """(fls (40, 18, 204), aus (40, 18, 80), face_id (1, 204)) in float64: a smooth random walk around a face, so that lip
    heights, motions and Laplacians are all away from zero"""
    g = torch.Generator().manual_seed(SEED + 1)
    face = torch.randn(1, 204, generator=g, dtype=torch.float64) * 0.3
    walk = torch.cumsum(torch.randn(N_WIN + 18, 204, generator=g, dtype=torch.float64) * 0.02, 0) + face
    fls = torch.stack([walk[i:i + 18] for i in range(N_WIN)])
    aus = torch.randn(N_WIN, 18, 80, generator=g, dtype=torch.float64)
    return fls, aus, walk[7:8].clone()


def main():
    import types
    import warnings
    warnings.filterwarnings('ignore')
    sys.path.insert(0, '/root/reference/Module1')
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    from src.models.model_audio2landmark import Audio2landmark_content
    import src.approaches.train_content as approach
    from src.dataset.audio2landmark.audio2landmark_dataset import Audio2landmark_Dataset
    from make_golden import save
    from make_module1_golden import seeded_state
    approach.device = torch.device('cpu')
    out = {}

    # ---- the windows of a 60-frame clip: frame t carries the value t, so a window's first column is its indices
    ds = types.SimpleNamespace(num_window_frames=18, num_window_step=1)
    frames = np.arange(60, dtype=np.float64).reshape(60, 1)
    fls_w, aus_w = Audio2landmark_Dataset.my_collate_in_segments_noemb(ds, [((frames * np.ones((1, 204)), None), (frames * np.ones((1, 80)), None))])
    assert torch.equal(fls_w[:, :, 0], aus_w[:, :, 0])
    out['win_index'] = fls_w[:, :, 0].numpy().astype(np.int64)

    # ---- loss, gradients and one Adam step per option combination
    fls, aus, face_id = segment_inputs()
    out.update(fls=fls, aus=aus, face_id=face_id, seed=np.int64(SEED), combos=np.array(COMBOS, dtype=np.int64))
    names = None
    for lip, motion in COMBOS:
        net = Audio2landmark_content(num_window_frames=18, in_size=80, use_prior_net=True, hidden_size=256, num_layers=3,
                                     drop_out=0, bidirectional=False)
        ks = [(k, tuple(v.shape), str(v.dtype)) for k, v in net.state_dict().items()]
        net.load_state_dict(seeded_state(ks, seed=SEED), strict=True)
        net.double().train()
        me = types.SimpleNamespace(C=net, opt_C=torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-6),
                                   opt_parser=types.SimpleNamespace(use_lip_weight=bool(lip), use_motion_loss=bool(motion),
                                                                    lambda_laplacian_smooth_loss=1.0))
        _, _, loss = approach.Audio2landmark_model.__train_content__(me, fls.clone(), aus.clone(), face_id.clone(), True)
        params = list(net.named_parameters())
        if names is None:
            names = [k for k, _ in params]
            out['param_names'] = np.array(names)
            out['param_sizes'] = np.array([p.numel() for _, p in params], dtype=np.int64)
        tag = 'lip%d_motion%d_' % (lip, motion)
        out[tag + 'loss'] = np.float64(loss.item())
        out[tag + 'grad_norm'] = np.array([float(p.grad.norm()) for _, p in params])
        out[tag + 'grad_samples'] = np.stack([p.grad.reshape(-1)[sample_index(p.numel())].numpy() for _, p in params])
        out[tag + 'adam_norm'] = np.array([float(p.detach().norm()) for _, p in params])
        out[tag + 'adam_samples'] = np.stack([p.detach().reshape(-1)[sample_index(p.numel())].numpy() for _, p in params])
        print(tag, 'loss %.9f' % loss.item())
    save('module1_train.npz', **out)


if __name__ == '__main__':
    main()
