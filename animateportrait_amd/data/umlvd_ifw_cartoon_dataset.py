"""The reference's cartoon training dataset (Module2/data/umlvd_ifw_cartoon_dataset.py:111-335 UMLVDIFWCartoonDataset) with
the batch prepared on the device: UMLVDIFWDataset (umlvd_ifw_dataset.py) with the differences the reference has between the two
files, and nothing else:

  * the files that go with a B image are found by replacing ``/Cartoon/`` (:153-170, :249), the static picture of a photo lies
    under ``/fakeB5_static/`` (:303) and is read when ``warp_loss == 2 or identity_loss == 2`` (:301);
  * the B side has no ``scanner_frag_*`` clips: no B1 / B2 items, no get_params3 draws, no select_target12 branch (:210-211).
    ``plan_sample`` therefore draws, in this order: the B index; get_params2 for A and for B; the branch draw r; the offsets of
    its branch -- the call sequence on ``random`` / ``torch.rand`` is the contract, as for the drawing dataset;
  * B (and the static picture) is RGB when ``output_nc == 3`` -- the parent's ``grayscale=(output_nc == 1)``.

``--coherent`` / ``--coh_use_more`` need the clips (:287-299 would index a list the reference's cartoon class never builds), so
they are refused here by name.  Image preparation is the parent's: ``apd_image_prep_u8`` launches, or ``--data_prep host``."""
from .umlvd_ifw_dataset import UMLVDIFWDataset


class UMLVDIFWCartoonDataset(UMLVDIFWDataset):
    B_FOLDER, STATIC_FOLDER, HAS_CLIPS = '/Cartoon/', '/fakeB5_static/', False

    def __init__(self, opt):
        if getattr(opt, 'coherent', 0) or getattr(opt, 'coh_use_more', 0):
            raise NotImplementedError('umlvd_ifw_cartoon: --coherent / --coh_use_more read frames of the scanner_frag_* video clips, '
                                      'which the cartoon data does not have (the cartoon model defaults both to 0)')
        UMLVDIFWDataset.__init__(self, opt)
