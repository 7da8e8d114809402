"""``--model geomcgt_ifw_test`` on the MI355X: the streaming-inference model of
Module2/models/geomcgt_ifw_test_model.py (options :178-189, __init__ :191-229, set_input :254-274,
forward :276-302), the caller that ``main_end2end_module2.py:96-97`` runs once per video frame.

What is the same: option names / defaults, ``netG_A`` through ``networks.define_G`` with ``--netg_resb_div/disp``, the
static drawing generator ``define_G(3, 1, 64, 'resnet_style2_9blocks', 'instance')`` for experiment names that contain
'drawing', the visual names, and every formula of ``forward`` (matte threshold, foreground compositing of the photo,
512^2 static drawing resized to 256^2, hot-path generator, ``grid_sample(mask, warp_motion, align_corners=True)``
blend of the animated foreground over the static drawing).

What is different (and why):
* The frozen third-party nets have no checkpoints in the reference tree: MODNet (matte)
  and netF (intrinsic flow) enter through ``self.aux`` callables; absent, their outputs are read from the input
  dict (``matte`` or ``mask``, ``iw_flow`` / ``if_mask``), as in the training model.
* The static drawing depends on the photo only, and the photo is constant over a clip: it is computed once per
  distinct ``real_A`` tensor and cached, where the reference recomputes it per frame.
* Batched: every formula is applied per sample (the reference is written for batch size 1).
* Experiment names that contain 'cartoon' (:228-229, 286-291): the reference round-trips the photo through uint8 and calls
  ``Photo2Cartoon.inference2(img, nocrop=1)`` (photo2cartoon.py:569-600).  On that branch the segmentation mask is computed
  and never applied, the 256 -> 256 resize is the identity and nothing is cropped or detected, so the static cartoon is
  exactly ``ResnetGenerator(ngf=32, img_size=256, light=True)(q(real_A))[0]`` with ``q`` the uint8 round trip
  ``floor((x + 1) 127.5) / 127.5 - 1`` -- networks.Photo2CartoonGenerator, loaded from ``checkpoints/static/cartoon.pt``
  (key ``genA2B``).  No TensorFlow, dlib or face_alignment is involved.  The input contract is [-1, 1]: a value outside is
  clamped to the byte range, where numpy's cast would wrap it.  Per sample, where the reference reads ``real_A[0]``.
"""
import torch

from .. import losses, networks, ops
from .base_model import BaseModel


class GeomCGTIFWTestModel(BaseModel):
    @staticmethod
    def modify_commandline_options(parser, is_train=True):                          # :178-189
        parser.set_defaults(no_dropout=True)
        parser.add_argument('--netg_resb_div', type=int, default=3, help='div')
        parser.add_argument('--netg_resb_disp', type=int, default=1, help='disp')
        parser.add_argument('--truncate', type=float, default=0.0, help='whether truncate in forward')
        parser.set_defaults(dataset_mode='umlvdfw_test')
        parser.add_argument('--draw_op', type=int, default=0, help='use which format to draw landmark')
        parser.add_argument('--blendbg', type=int, default=0, help='whether blend with bg')
        return parser

    def __init__(self, opt):
        BaseModel.__init__(self, opt)
        self.visual_names = ['real_A', 'real_A_lm', 'target_B_lm', 'fake_B', 'fake_B_vis', 'fg_mask', 'fakeB_static',
                             'fake_B_fore', 'fg_mask1']                            # :199-204
        self.model_names = ['G_A']
        gid = [self.gpu_ids[0]]
        self.netG_A = networks.define_G(opt.input_nc, opt.output_nc, opt.ngf, opt.netG, opt.norm, not opt.no_dropout,
                                        opt.init_type, opt.init_gain, gid, div=opt.netg_resb_div,
                                        disp=opt.netg_resb_disp)                   # :211-213
        self.aux = {'modnet': None, 'netF': None}
        self.cartoon = 'cartoon' in opt.name
        if self.cartoon:
            # the static cartoon generator of the Photo2Cartoon project, frozen                        :228-229
            self.net_staticG = networks.Photo2CartoonGenerator(ngf=32, img_size=256, light=True).to(self.device)
            self.STATIC_CHECKPOINT = 'checkpoints/static/cartoon.pt'
        else:
            # 'drawing' (the README / main_end2end configuration): static generator, frozen           :224-227
            self.net_staticG = networks.define_G(3, 1, 64, 'resnet_style2_9blocks', 'instance', use_dropout=False,
                                                 gpu_ids=gid)
        self.net_staticG.eval()
        self._static_key = None
        self._style = None
        self._static_loaded = False

    STATIC_CHECKPOINT = 'checkpoints/static/drawing.pth'                              # :226

    def setup(self, opt):
        """base_model.py:79-90 plus the static generator's checkpoint, which the reference loads unconditionally in
        __init__ (:226).  A missing file is an error unless --allow_random_init (smoke mode) is set."""
        if not self._static_loaded:
            import os
            if os.path.exists(self.STATIC_CHECKPOINT):
                self.load_static(self.STATIC_CHECKPOINT)
            elif not getattr(opt, 'allow_random_init', False):
                raise FileNotFoundError('%s (static %s generator) not found; load it with load_static(path) '
                                        'before setup() or pass --allow_random_init'
                                        % (self.STATIC_CHECKPOINT, 'cartoon' if self.cartoon else 'drawing'))
            else:
                print('WARNING: --allow_random_init: static %s generator runs with RANDOM weights'
                      % ('cartoon' if self.cartoon else 'drawing'))
        BaseModel.setup(self, opt)

    def load_static(self, path):
        """checkpoints/static/drawing.pth (:226), or checkpoints/static/cartoon.pt's ``genA2B`` entry (:229,
        photo2cartoon.py:534-535): same key names, strict."""
        sd = torch.load(path, map_location=self.device)
        if self.cartoon:
            sd = sd['genA2B']
        self.net_staticG.load_state_dict(sd, strict=True)
        self._static_key = None
        self._static_loaded = True

    # ------------------------------------------------------------------------------------------------ input
    def set_input(self, input):                                                      # :254-274
        AtoB = self.opt.direction == 'AtoB'
        dev = self.device
        photo = input['A' if AtoB else 'B']
        self._photo_key = (id(photo), photo._version, tuple(photo.shape))   # a clip passes the same photo tensor per frame
        self._photo_ref = photo                                             # (kept alive so that its id stays unique)
        self.real_A = photo.to(dev)
        self.warp_motion = input['warp_motion'].to(dev)
        alm = input['A_lm']
        self.real_A_lm = alm.to(dev)
        # The photo's landmark map is constant over a clip.  A streaming caller that guarantees it (ClipStreamer: one tensor
        # per batch size, never written to) names the clip with ``input['clip_id']``; its encoding inside the generator is then
        # cached under (clip id, shape, arithmetic mode).  Without a clip id -- dataset runs, bench steps -- there is no cache:
        # both landmark maps run through the encoder as one 2B pass.
        cid = input.get('clip_id')
        self.netG_A.land1_cache_key = None if cid is None else (cid, tuple(alm.shape), ops.DEFAULT_PRECISION)
        self.target_B_lm = input['tB_lm'].to(dev)
        for k, attr in (('realA_static_warp', 'realA_static_warp'), ('A_lm_68', 'real_A_lm_68'),
                        ('tB_lm_68', 'target_B_lm_68'), ('winB', 'winB')):
            if k in input:
                setattr(self, attr, input[k].to(dev) if torch.is_tensor(input[k]) else input[k])
        self.image_paths = input.get('image_paths')
        if self.aux['netF'] is not None:
            self.iw_flow, self.real_A_if_mask = losses.flow_network_warp(                       # :62-76, :270-271
                self.aux['netF'], self.real_A, self.real_A_lm_68[:, :68], self.target_B_lm_68[:, :68])
        elif 'iw_flow' in input and 'if_mask' in input:
            self.iw_flow, self.real_A_if_mask = input['iw_flow'].to(dev), input['if_mask'].to(dev)
        else:
            raise RuntimeError('geomcgt_ifw_test: the input carries no iw_flow / if_mask and no flow network is attached: load '
                               'the intrinsic-flow checkpoint (netF) into model.aux[\'netF\']')
        self._matte_in = None
        if self.aux['modnet'] is None:
            if 'matte' not in input and 'mask' not in input:
                raise RuntimeError('geomcgt_ifw_test: the input carries no matte / mask and no matting network is attached: '
                                   'load the MODNet checkpoint into model.aux[\'modnet\']')
            self._matte_in = (input['matte'] if 'matte' in input else input['mask']).to(dev)

    # ------------------------------------------------------------------------------------------------ forward
    def static_drawing(self, real_A):
        """:280-291, cached per photo.  Drawing: style planes (0, 1, 0) at 128^2, 256 -> 512 -> G_static -> 256.
        Cartoon: the unmasked photo through the uint8 round trip, G_static at 256^2, (N, 3, 256, 256)."""
        key = self._photo_key
        if self._static_key != key and self.cartoon:
            # :286-291 with inference2(nocrop=1) reduced to what it computes: G(q(photo)) at 256^2, the tanh image as it is
            from .. import style_ops
            self.fakeB_static = self.net_staticG(style_ops.quantize_u8(real_A).contiguous())
            self._static_key = key
        elif self._static_key != key:
            n = real_A.shape[0]
            if self._style is None or self._style.shape[0] != n:
                self._style = torch.tensor([0., 1., 0.], device=real_A.device).view(1, 3, 1, 1).repeat(n, 1, 128, 128)
            a512 = ops.resize_bilinear(real_A.contiguous(), (512, 512))
            y512 = self.net_staticG(a512, self._style)
            self.fakeB_static = ops.resize_bilinear(y512, (256, 256))
            self._static_key = key
        return self.fakeB_static

    def forward(self):                                                               # :276-302
        if self.aux['modnet'] is not None:
            _, _, matte = self.aux['modnet'](self.real_A, True)
        else:
            matte = self._matte_in
        mask = (matte > 0.5).float()
        fakeB_static = self.static_drawing(self.real_A)       # of the unmasked photo, as :282-285
        self.real_A = losses.fore_composite(self.real_A, mask)
        self.fg_mask = (mask * 2 - 1).repeat(1, 3, 1, 1)
        with torch.no_grad():
            self.fake_B = self.netG_A(self.real_A.contiguous(), self.real_A_lm, self.target_B_lm, self.warp_motion,
                                      self.iw_flow, self.real_A_if_mask)
        self.mask1 = ops.grid_sample(mask.contiguous(), self.warp_motion.contiguous(), align_corners=True)
        self.fake_B_fore = self.fake_B.clone()
        self.fake_B = losses.bg_blend(self.fake_B, fakeB_static, self.mask1)
        self.fg_mask1 = (self.mask1 * 2 - 1).repeat(1, 3, 1, 1)
        if hasattr(self, 'target_B_lm_68') and hasattr(self, 'winB'):
            self.fake_B_vis = self.get_lmvis(self.fake_B, self.target_B_lm_68, self.winB)

    def get_lmvis(self, tensor_im, lm, win, hradius=3):                             # :232-251
        """The frame with its landmarks and window marked red, one apd_landmark_marks launch for the batch.  The reference
        is written for batch size 1; here every sample gets its own marks, and boxes are clipped to the image."""
        from ..data import visuals
        return visuals.landmark_marks(tensor_im, lm, win, hradius)

    def optimize_parameters(self):
        pass                                                                         # test-time model
