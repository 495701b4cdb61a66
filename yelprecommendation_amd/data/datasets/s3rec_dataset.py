"""S3Rec dataset — drop-in for reference data/datasets/s3rec_dataset.py:8-57, plus the way to the device path.

``S3RecDataset(data, item2attribute, attributes_count, num_items, train)[user]`` returns the reference's dict:
``user_id``, ``X``, and ``pos_items`` + ``neg_items`` (one negative per position, pads included) when ``train``,
``pos_item`` (= ``Y[-1]``) + ``neg_items`` (99 mutually distinct negatives) otherwise.  Negatives come from the same
rejection loop over the global NumPy RNG — ``np.random.randint(1, num_items + 1)`` redrawn while the value is in the
user's ``behaviors`` or already taken — the same calls in the same order, so a seeded host run replays the reference's
stream.

Two things to know:

* The reference tests its 1-based draw against the raw 0-based ``behaviors`` list — an off-by-one of its own: the
  value v is refused when the user has the item whose 1-based id is v + 1.  It is kept, here and (by default) on the
  device path, so that both sample from the reference's distribution.
* ``aap_actual`` / ``mip_actual`` are left out.  Only the reference's pre-training reads them; ``S3RecPreTrainer``
  takes its targets from ``X`` and an item -> categories CSR instead.  ``mip_actual`` alone is ``max_seq_len x
  (num_items + 1)`` doubles per user, and building them draws no random numbers: leaving them out moves nothing in the
  RNG stream.

``to_sequences(device, max_seq_len)`` hands the same behaviour rows to :class:`...s3rec_batches.S3RecSequences`.
"""
import numpy as np
from torch.utils.data import Dataset


class S3RecDataset(Dataset):

    def __init__(self, data, item2attribute=None, attributes_count=None, num_items=None, train=True):
        super().__init__()
        self.data = data
        self.num_items = num_items
        self.train = train
        self.item2attribute = item2attribute
        self.attributes_count = attributes_count
        # column arrays once, instead of a pandas .iloc per user
        self._X, self._Y, self._behaviors = data['X'].values, data['Y'].values, data['behaviors'].values

    def __len__(self):
        return self.data.shape[0]

    def _negative_sampling(self, behaviors):
        # reference s3rec_dataset.py:21-29
        sample_size = 1 if self.train else 99
        neg_items = []
        for _ in range(sample_size):
            neg_item = np.random.randint(1, self.num_items + 1)
            while (neg_item in behaviors) or (neg_item in neg_items):
                neg_item = np.random.randint(1, self.num_items + 1)
            neg_items.append(neg_item)
        return neg_items

    def __getitem__(self, user_id):
        # reference s3rec_dataset.py:31-57 without aap_actual / mip_actual
        pos_items = np.array(self._Y[user_id], dtype='int64')
        behaviors = self._behaviors[user_id]
        if self.train:
            return {
                'user_id': user_id,
                'X': np.array(self._X[user_id], dtype='int64'),
                'pos_items': pos_items,
                'neg_items': np.array([self._negative_sampling(behaviors)[0] for _ in range(pos_items.shape[0])]),
            }
        return {
            'user_id': user_id,
            'X': np.array(self._X[user_id], dtype='int64'),
            'pos_item': pos_items[-1],
            'neg_items': np.array(self._negative_sampling(behaviors), dtype='int64'),
        }

    def to_sequences(self, device, max_seq_len, seed=0, shifted=False):
        """Device-side batch builder over the same behaviour rows (user = row position, as ``__getitem__`` indexes)."""
        from ..s3rec_batches import S3RecSequences
        return S3RecSequences.from_frame(self.data, self.num_items, max_seq_len, device, seed=seed, shifted=shifted)
