"""Dataset registry (Module2/data/__init__.py:47-91).

``umlvd_ifw`` is the reference's training dataset on its own file tree, with the batch prepared on the device
(umlvd_ifw_dataset.py); ``synthetic`` produces batches with the same dict keys / shapes / value ranges from a seed and needs
no files.  The reference's test-time dataset (umlvdfw_test) is not here: test.py drives the generator from frames."""
from .synthetic_dataset import SyntheticDataset


def find_dataset_using_name(name):
    if name == 'synthetic':
        return SyntheticDataset
    if name == 'umlvd_ifw':
        from .umlvd_ifw_dataset import UMLVDIFWDataset
        return UMLVDIFWDataset
    raise NotImplementedError('dataset_mode [%s] is not implemented; use --dataset_mode umlvd_ifw (the reference\'s training '
                              'tree) or --dataset_mode synthetic' % name)


def get_option_setter(name):
    if name in ('synthetic', 'umlvd_ifw'):
        return find_dataset_using_name(name).modify_commandline_options
    return lambda parser, is_train: parser   # unknown modes fail in create_dataset, with the message above


def create_dataset(opt):
    return find_dataset_using_name(opt.dataset_mode)(opt)
