"""DCN dataset — drop-in for reference data/datasets/dcn_dataset.py: the MF triplets (the attributes are looked up
by item id on the device inside the model step)."""
from .mf_dataset import MFDataset


class DCNDataset(MFDataset):
    def __init__(self, data, num_items=None):
        super().__init__(data, num_items)
