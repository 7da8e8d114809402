"""Dataset registry (Module2/data/__init__.py:47-91).

``umlvd_ifw`` is the reference's training dataset on its own file tree, with the batch prepared on the device
(umlvd_ifw_dataset.py); ``umlvdfw_test`` is its test-time dataset on the same tree (umlvdfw_test_dataset.py: photo,
both landmark maps, motion grid and static warp per batch, the default of ``--model geomcgt_ifw_test``);
``umlvd_ifw_cartoon`` is the cartoon style's training dataset (umlvd_ifw_cartoon_dataset.py: ``/Cartoon/`` siblings, no video
clips, RGB targets, the default of ``--model geomgm_ifw_cartoon_fore``); ``synthetic`` produces batches with the same dict keys / shapes / value ranges from a
seed and needs no files."""
from .synthetic_dataset import SyntheticDataset


def find_dataset_using_name(name):
    if name == 'synthetic':
        return SyntheticDataset
    if name == 'umlvd_ifw':
        from .umlvd_ifw_dataset import UMLVDIFWDataset
        return UMLVDIFWDataset
    if name == 'umlvd_ifw_cartoon':
        from .umlvd_ifw_cartoon_dataset import UMLVDIFWCartoonDataset
        return UMLVDIFWCartoonDataset
    if name == 'umlvdfw_test':
        from .umlvdfw_test_dataset import UMLVDFWTestDataset
        return UMLVDFWTestDataset
    raise NotImplementedError('dataset_mode [%s] is not implemented; use --dataset_mode umlvd_ifw (the reference\'s training '
                              'tree), umlvd_ifw_cartoon (its cartoon training tree), umlvdfw_test (its test tree) or '
                              '--dataset_mode synthetic' % name)


def get_option_setter(name):
    if name in ('synthetic', 'umlvd_ifw', 'umlvd_ifw_cartoon', 'umlvdfw_test'):
        return find_dataset_using_name(name).modify_commandline_options
    return lambda parser, is_train: parser   # unknown modes fail in create_dataset, with the message above


def create_dataset(opt):
    return find_dataset_using_name(opt.dataset_mode)(opt)
