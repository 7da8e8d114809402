"""Inference entry point -- counterpart of Module2/test.py:38-66: build the model, load ``G_A``, run the
generator over the dataset and write the frames.  ``--save_format npy`` (the default) writes ``fake_B`` as one ``.npy`` per
frame; ``png`` writes every visual of ``get_current_visuals()`` as ``<stem>_<label>.png``, the names the reference's
util/visualizer.py save_images gives, through the device sink of data/visuals.py; ``both`` does both.  ``--png_encoder device``
(with ``png`` / ``both``) makes the PNG files on the device (apd_png_encode) instead of in PIL on the host: the same pixels in
larger files.  The HTML page of the reference's visualizer is not written."""
import os

import numpy as np
import torch

from .data import create_dataset
from .models import create_model
from .options.base_options import TestOptions

SAVE_FORMATS = ('npy', 'png', 'both')
PNG_ENCODERS = ('host', 'device')


def parse(argv=None):
    """TestOptions plus --save_format and --png_encoder, which are this entry point's own flags"""
    options = TestOptions()
    initialize = options.initialize

    def with_save_format(p):
        p = initialize(p)
        p.add_argument('--save_format', type=str, default='npy', choices=SAVE_FORMATS,
                       help='npy: fake_B per frame as .npy; png: every visual as <stem>_<label>.png; both')
        p.add_argument('--png_encoder', type=str, default='host', choices=PNG_ENCODERS,
                       help='with --save_format png|both: host = PIL on a thread pool; device = the files are encoded on the GPU '
                            '(fixed-Huffman deflate: same pixels, larger files) and the host only writes them')
        return p
    options.initialize = with_save_format
    return options.parse(argv)


def main(argv=None, prepare_model=None):
    """``prepare_model(model)`` runs after the model is built and before setup(): the place to attach the frozen third-party
    networks (model.aux) the reference loads from checkpoints this project does not ship."""
    opt = parse(argv)
    opt.num_threads, opt.serial_batches, opt.no_flip = 0, True, True     # test.py:41-45
    torch.cuda.set_device(opt.gpu_ids[0])
    dataset = create_dataset(opt)
    model = create_model(opt)
    if prepare_model is not None:
        prepare_model(model)
    model.setup(opt)       # loads '<epoch>_net_G_A.pth'; a missing file is an error (test.py:48) unless --allow_random_init
    if opt.eval:
        model.eval()
    out_dir = os.path.join(opt.results_dir, opt.name, '%s_%s' % (opt.phase, opt.epoch), opt.imagefolder)
    os.makedirs(out_dir, exist_ok=True)
    n = 0
    for data in dataset:
        if n >= opt.num_test:
            break
        model.set_input(data)
        model.test()
        paths = [str(p) for p in model.get_image_paths()]
        if opt.save_format in ('npy', 'both'):
            fake = model.fake_B.detach().cpu().numpy()
            for i, path in enumerate(paths):
                np.save(os.path.join(out_dir, os.path.basename(path) + '_fake_B.npy'), fake[i])
        if opt.save_format in ('png', 'both'):
            from .data import visuals
            stems = [os.path.splitext(os.path.basename(path))[0] for path in paths]
            shown = {label: t for label, t in model.get_current_visuals().items() if torch.is_tensor(t) and t.dim() == 4}
            visuals.save_png_batch(shown, {label: [os.path.join(out_dir, '%s_%s.png' % (s, label)) for s in stems] for label in shown},
                                   encoder=opt.png_encoder)
        n += len(paths)
    print('wrote %d frames to %s' % (n, out_dir))


if __name__ == '__main__':
    main()
