"""DCN data pipeline — drop-in for reference data/datasets/dcn_data_pipeline.py:9-47.

The MF split and triplet stream (``DCNDataPipeline(MFDataPipeline)``) plus the item attributes of
``<data_dir>/yelp_item2attributes.json``, read as the reference reads them: ``pd.read_json(...).transpose()``,
``attributes_count = [categories.explode().nunique(), statecity.nunique()]``, the category lists padded with -1 to
the longest list and shifted by +1 (slot 0 is padding).  ``item2attributes`` is the reference's dict; ``cat_ids``
(int32 [num_items, Lmax]) and ``sc_ids`` (int32 [num_items]) are the same table on the device, what the kernels
gather from instead of per-item dict lookups.
"""
import os

import numpy as np
import pandas as pd

from ...utils import logger
from .mf_data_pipeline import MFDataPipeline


class DCNDataPipeline(MFDataPipeline):

    def __init__(self, cfg):
        super().__init__(cfg)
        self.item2attributes = None
        self.attributes_count = None
        self.cat_ids = None
        self.sc_ids = None

    def preprocess(self) -> pd.DataFrame:
        logger.info("start preprocessing...")
        df = self._load_df()
        self._set_num_items_and_num_users(df)
        if self.cfg.loss_name == 'pointwise':
            raise NotImplementedError("pointwise negative sampling is outside the BPR path")
        self.item2attributes = self._load_attributes()
        logger.info("done")
        return df

    def _read_attributes(self) -> pd.DataFrame:
        return pd.read_json(os.path.join(self.cfg.data_dir, 'yelp_item2attributes.json')).transpose()

    def _load_attributes(self):
        # reference dcn_data_pipeline.py:29-40
        logger.info("load item2attributes...")
        df = self._read_attributes()
        self.attributes_count = [df.categories.explode().nunique(), df.statecity.nunique()]
        max_len = df.categories.apply(len).max()
        df.categories = df.categories.apply(lambda x: list(x) + [-1] * (max_len - len(x)))
        df.categories = df.categories.apply(lambda x: [y + 1 for y in x])
        self._set_device_tables(df, max_len)
        return df.transpose().to_dict()

    def _set_device_tables(self, df, max_len):
        import torch
        items = np.asarray(df.index.values, dtype=np.int64)
        n = self.num_items if self.num_items is not None else int(items.max()) + 1
        if len(items) != n or not np.array_equal(np.sort(items), np.arange(n)):
            raise ValueError(f"item attributes must cover the item ids 0..{n - 1} exactly")
        cats = np.zeros((n, max_len), dtype=np.int32)
        cats[items] = np.array(df.categories.tolist(), dtype=np.int32).reshape(len(items), max_len)
        sc = np.zeros(n, dtype=np.int32)
        sc[items] = df.statecity.values.astype(np.int32)
        dev = self.cfg.device if str(self.cfg.device).lower() != "cuda" or torch.cuda.is_available() else "cpu"
        self.cat_ids = torch.from_numpy(cats).to(dev)
        self.sc_ids = torch.from_numpy(sc).to(dev)


DCNDatapipeline = DCNDataPipeline          # the reference's spelling
