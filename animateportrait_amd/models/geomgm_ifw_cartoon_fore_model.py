"""``--model geomgm_ifw_cartoon_fore`` on the MI355X: the training model of the cartoon style
(Module2/models/geomgm_ifw_cartoon_fore_model.py), as what it is in the reference -- the drawing model
(geomgm_ifw_fore_model.py) with a 3-channel frame and a handful of differences:

* defaults ``--dataset_mode umlvd_ifw_cartoon``, ``--coherent 0``, ``--coh_use_more 0`` (:165, :195, :197): the cartoon data
  has no video clips, so there is no coherence discriminator by default;
* no ``--select_target12_thre`` and no ``--rx / --ry / --rs`` (:200, :203): the video branch does not exist;
* ``visual_names`` without ``real_A_fore`` and without the ``blendbg == 2`` entry (:223-230);
* the identity loss compares LUMINANCE planes: ``0.299 R + 0.587 G + 0.114 B`` of the generated frame and of the static
  cartoon (:745-748), one HIP launch each way (losses.luminance) -- networks.FaceLoss then reads that plane three times
  itself, the path the 1-channel drawing takes.

Checkpoint keys, option names, ``model_names`` and ``loss_names`` are the reference's; everything else (batched semantics, 2B
launches, aux-net slots, the order G step then D step) is inherited from GeomGMIFWForeModel."""
from .. import losses, networks
from .geomgm_ifw_fore_model import GeomGMIFWForeModel


class GeomGMIFWCartoonForeModel(GeomGMIFWForeModel):
    DATASET_MODE = 'umlvd_ifw_cartoon'
    COHERENT, COH_USE_MORE = 0, 0
    VIDEO_TARGET_OPTIONS = False

    def __init__(self, opt):
        GeomGMIFWForeModel.__init__(self, opt)
        self.loss_names, self.visual_names = self.reference_names(opt, self.isTrain)

    @staticmethod
    def reference_names(opt, is_train):
        """``loss_names`` and ``visual_names`` in the reference's order (:217-280)."""
        loss = ['D_A', 'G_A', 'geom_B']
        vis = ['real_A', 'realA_static_warp', 'realA_static_warp2', 'real_A_lm', 'target_B_lm', 'fake_B', 'target_B2_lm', 'fake_B2']
        if is_train:
            vis = ['real_A', 'realA_static_warp', 'realA_static_warp2', 'real_A_if_face', 'real_A_if_mask', 'real_A_lm',
                   'target_B_lm', 'fake_B', 'fake_B_lm_68_vis', 'fake_B_lm_68_vist', 'target_B2_lm', 'fake_B2',
                   'fake_B2_lm_68_vis', 'fake_B2_lm_68_vist']
        if opt.blendbg:
            vis += ['fake_B_fore', 'fake_B2_fore', 'mask', 'mask1', 'mask2']
        if is_train and opt.lambda_geom_lipline > 0:
            vis += ['liplinemask1', 'liplinemask2']
            loss += ['geom_B_lipline']
        if is_train and opt.warp_loss:
            vis += ['fakeB_static'] if opt.warp_loss == 2 else []
            vis += ['fakeB_static_warp']
            loss += ['warp_B']
        if is_train:
            vis += ['fake_B_warp']
            loss += ['warp_inter1']
        if is_train and opt.identity_loss:
            loss += ['iden_B']
        if is_train and opt.coherent:
            vis += ['real_B1_lm_68_vist', 'real_B2_lm_68_vist']
            vis += ['real_B3', 'real_B4'] if opt.coh_use_more else []
            loss += ['D_A_coh', 'G_A_coh']
        for flag, suf in ((opt.use_mask, ''), (opt.use_eye_mask, 'e'), (opt.use_lip_mask, 'l')):
            if is_train and flag:
                vis += ['fake_B_l' + suf, 'fake_B2_l' + suf, 'real_B_l' + suf]
                loss += ['D_A_l' + suf, 'G_A_l' + suf]
        if is_train:
            loss += ['G']
        for flag, suf in ((opt.use_mask, ''), (opt.use_eye_mask, 'e'), (opt.use_lip_mask, 'l')):
            if not is_train and flag:
                vis += ['fake_B_l' + suf, 'real_B_l' + suf]
        return loss, vis + ['real_B', 'real_B_lm']

    def identity_pair(self, fl):
        """:736-749 with a colour frame: the generated cartoon enters as its luminance plane; its partner is the photo's
        luminance (--identity_loss 1) or the static cartoon's (2).  A 1-channel frame (--output_nc 1) is its own luminance."""
        gray = lambda x: losses.luminance(x) if x.shape[1] == 3 else x          # noqa: E731
        rep = (lambda x: x) if isinstance(fl, networks.FaceLoss) else (lambda x: x.repeat(1, 3, 1, 1))   # noqa: E731
        other = self.real_A if self.opt.identity_loss == 1 else self.fakeB_static
        return rep(gray(self.fake_B)), rep(gray(other.detach()))
