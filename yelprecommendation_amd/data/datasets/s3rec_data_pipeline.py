"""S3Rec data pipeline — drop-in for reference data/datasets/s3rec_data_pipeline.py:6-92.

``preprocess()`` groups the interactions by user into one ``behaviors`` list per user (frame order, repeats kept)
and reads the item attributes; ``split(df)`` cuts every list into the three (X, Y) windows the reference cuts
(train ``row[:-3]`` / ``row[1:-2]``, valid ``row[:-2]`` / ``row[2:-1]``, test ``row[:-1]`` / ``row[3:]``), each brought
to ``cfg.max_seq_len`` by ``_adjust_seq_len``: the last entries kept, -1 padded on the left, then everything + 1, so
that 0 is the pad and the items are 1..num_items.  The frames feed :class:`.s3rec_dataset.S3RecDataset` (the host
path) and :class:`...s3rec_batches.S3RecSequences` (the device path, which restates the same windows in
csrc/s3rec_batches.hip).
"""
import os

import pandas as pd

from ...utils import logger
from .data_pipeline import DataPipeline


class S3RecDataPipeline(DataPipeline):

    def __init__(self, cfg):
        super().__init__(cfg)
        self.num_users = None
        self.num_items = None
        self.item2attributes = None
        self.attributes_count = None

    def split(self, df: pd.DataFrame):
        # reference s3rec_data_pipeline.py:13-37
        train_df_X = df.behaviors.apply(lambda row: row[:-3]).rename('X')
        train_df_Y = df.behaviors.apply(lambda row: row[1:-2]).rename('Y')
        valid_df_X = df.behaviors.apply(lambda row: row[:-2]).rename('X')
        valid_df_Y = df.behaviors.apply(lambda row: row[2:-1]).rename('Y')
        test_df_X = df.behaviors.apply(lambda row: row[:-1]).rename('X')
        test_df_Y = df.behaviors.apply(lambda row: row[3:]).rename('Y')

        train_df_X = self._adjust_seq_len(train_df_X)
        valid_df_X = self._adjust_seq_len(valid_df_X)
        test_df_X = self._adjust_seq_len(test_df_X)

        train_df_Y = self._adjust_seq_len(train_df_Y)
        valid_df_Y = self._adjust_seq_len(valid_df_Y)
        test_df_Y = self._adjust_seq_len(test_df_Y)

        return pd.concat([df, train_df_X, train_df_Y], axis=1), \
            pd.concat([df, valid_df_X, valid_df_Y], axis=1), \
            pd.concat([df, test_df_X, test_df_Y], axis=1)

    def _adjust_seq_len(self, df):
        # reference s3rec_data_pipeline.py:40-50
        def _adjust_seq_len_by_user(row):
            if len(row) > self.cfg.max_seq_len:
                row = row[-self.cfg.max_seq_len:]
            elif len(row) < self.cfg.max_seq_len:
                row = [-1] * (self.cfg.max_seq_len - len(row)) + row
            # item 0: pad, item starts from 1
            return [e + 1 for e in row]

        return df.apply(_adjust_seq_len_by_user)

    def preprocess(self) -> pd.DataFrame:
        # reference s3rec_data_pipeline.py:53-71: one row per user, column 'behaviors'
        logger.info("start preprocessing...")
        df = self._load_df()
        self._set_num_items_and_num_users(df)
        df = df.groupby(['user_id']).agg({'business_id': [('behaviors', list)]}).droplevel(0, 1)
        self.item2attributes = self._load_attributes()
        logger.info(f"item2attributes : {len(self.item2attributes)}")
        logger.info("done")
        return df

    def _load_df(self):
        logger.info("load df...")
        return pd.read_csv(os.path.join(self.cfg.data_dir, 'yelp_interactions.tsv'), sep='\t', index_col=False)

    def _read_attributes(self) -> pd.DataFrame:
        return pd.read_json(os.path.join(self.cfg.data_dir, 'yelp_item2attributes.json')).transpose()

    def _load_attributes(self):
        # reference s3rec_data_pipeline.py:79-87: {item + 1: {'categories': [...]}} and the pad's empty entry
        logger.info("load item2attributes...")
        df = self._read_attributes()
        self.attributes_count = df.categories.explode().nunique()
        df = df.drop(columns=['statecity']).transpose().to_dict()
        df = {key + 1: value for key, value in df.items()}
        df.update({0: {'categories': []}})
        return df

    def _set_num_items_and_num_users(self, df):
        self.num_items = df.business_id.nunique()
        self.num_users = df.user_id.nunique()
