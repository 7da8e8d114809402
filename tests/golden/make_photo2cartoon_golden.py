#!/usr/bin/env python3
"""Golden outputs of the static cartoon generator from the REFERENCE's own ``ResnetGenerator(ngf, img_size, light=True)``
(Module2/models/photo2cartoon.py:166-525), imported read-only.  That file imports cv2, tensorflow
(``tensorflow.python.platform.gfile``) and face_alignment at its top for its face detection / segmentation classes; none is
installed here and none is used by the generator class, so empty stand-in modules take their place in ``sys.modules``.

Written to tests/golden/photo2cartoon.npz: the state_dict's key names and shapes at ngf 8 and ngf 32, the seeds, a sha256 of the
ngf-8 weights (tests/photo2cartoon_reference.py: init_params), the input (N = 2, 64 x 64), the tanh output of the batch and of
sample 0 alone.  The maker asserts that the output has a spread of at least 0.2 -- an absolute tolerance on a near-constant
image would show nothing -- and that the restatement in tests/photo2cartoon_reference.py reproduces the class.

    python tests/golden/make_photo2cartoon_golden.py          (build container only)
"""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = '/root/reference/Module2/models/photo2cartoon.py'
NGF, SIZE, N, SEED_W, SEED_X = 8, 64, 2, 2468, 97


def _stand_ins():
    for name in ('cv2', 'tensorflow', 'tensorflow.python', 'tensorflow.python.platform', 'tensorflow.python.platform.gfile',
                 'face_alignment'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['tensorflow.python.platform'].gfile = sys.modules['tensorflow.python.platform.gfile']


def sd_sha(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    import photo2cartoon_reference as pr
    _stand_ins()
    spec = importlib.util.spec_from_file_location('ref_photo2cartoon', REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {'ngf': np.array(NGF), 'size': np.array(SIZE), 'seed_w': np.array(SEED_W), 'seed_x': np.array(SEED_X)}
    for ngf in (8, 32):
        keys = [(k, tuple(v.shape)) for k, v in ref.ResnetGenerator(ngf=ngf, img_size=256, light=True).state_dict().items()]
        assert keys == [(k, tuple(s)) for k, s in pr.param_shapes(ngf)], 'param_shapes(%d) differs from the class' % ngf
        out['keys_ngf%d' % ngf] = np.array([k for k, _ in keys])
        out['shapes_ngf%d' % ngf] = np.array([','.join(map(str, s)) for _, s in keys])
    sd = pr.init_params(pr.param_shapes(NGF), SEED_W)
    net = ref.ResnetGenerator(ngf=NGF, img_size=SIZE, light=True).double().eval()
    net.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    x = torch.rand(N, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(SEED_X)) * 2 - 1
    with torch.no_grad():
        y = net(x.double())[0]
        y0 = net(x[:1].double())[0]
    spread = float(y.std())
    print('tanh output: std %.3f, min %.3f, max %.3f' % (spread, float(y.min()), float(y.max())))
    assert spread >= 0.2, 'the output is too flat for an absolute tolerance to mean anything'
    mine = pr.generator_forward(sd, x)
    err = float((mine - y).abs().max())
    print('restatement vs class (float64): L-inf %.3e;  sample 0 alone vs in the batch: %.3e' % (err, float((y0 - y[:1]).abs().max())))
    assert err < 1e-10
    out.update(weights_sha256=np.array(sd_sha(sd)), x=x.numpy(), y=y.float().numpy(), y0=y0.float().numpy(), spread=np.array(spread))
    path = os.path.join(HERE, 'photo2cartoon.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
