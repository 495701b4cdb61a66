"""Device-side S3Rec batches (the S3Rec counterpart of data/triplets.py) — csrc/s3rec_batches.hip through the C ABI.

The reference builds every S3Rec batch on the host: ``S3RecDataPipeline.split`` keeps three padded (X, Y) windows per
user (data/datasets/s3rec_data_pipeline.py:13-50) and ``S3RecDataset.__getitem__`` draws the negatives, one
``np.random.randint`` plus a Python ``in list`` test per draw — ``max_seq_len`` of them per training sequence, 99
mutually distinct ones per test sequence, for every user, every epoch (s3rec_dataset.py:21-57).  Here the behaviour
rows stay on the device as one CSR and ONE kernel launch produces the rows of any set of users: the windows are cut
from the CSR in the kernel, and a user's negatives are a pure function of (seed, epoch, mode, user) (Philox rejection
sampling, as in data/triplets.py), so there is no state, no host synchronisation, and any batch equals the same rows of
the whole epoch.  The generator differs from NumPy's stream by construction; the LAW is the reference's
(tests/s3rec_batches_ref.py states it on the CPU, word for word what the kernel gives).

What the negatives avoid.  The reference tests its 1-based draw against the raw 0-based ``behaviors`` list — an
off-by-one of its own.  By default the store reproduces it: a user's avoid values are the raw ids of the behaviour row
that fall in 1..num_items, so the host path and the device path sample from the same distribution.  ``shifted=True``
gives ``id + 1`` instead: the items the user really has.

Batches exist on the GPU only; on CPU tensors the store raises.
"""
import torch

from .. import engine

MODES = ("train", "valid", "test")


class S3RecSequences:
    """Per-user behaviour rows (CSR, raw 0-based item ids in interaction order, repeats kept) and avoid values (CSR,
    ascending and duplicate-free inside a user, in the draw space 1..num_items) on the device."""

    def __init__(self, user_id, item_id, num_users, num_items, max_seq_len, seed=0, shifted=False):
        """``user_id, item_id``: the interactions in interaction order (int64 tensors on the GPU; users are the dense
        ids 0..num_users-1 — the row positions of the pipeline's frame)."""
        if not user_id.is_cuda:
            raise engine.EngineError("S3RecSequences runs on the GPU only (csrc/s3rec_batches.hip); the host path is "
                                     "DataLoader(S3RecDataset)")
        self.device = user_id.device
        self.num_users, self.num_items, self.max_seq_len = int(num_users), int(num_items), int(max_seq_len)
        self.seed, self.shifted = int(seed), bool(shifted)
        user, item = user_id.long(), item_id.long().to(self.device)
        if user.numel() and not 0 <= int(user.min()) <= int(user.max()) < self.num_users:
            raise ValueError("S3RecSequences: user ids must be the dense ids 0..num_users-1")
        user, order = torch.sort(user, stable=True)                      # by user, interaction order inside a user
        self.beh_idx = item[order].contiguous()
        self.beh_ptr = torch.zeros(self.num_users + 1, dtype=torch.int64, device=self.device)
        self.beh_ptr[1:] = torch.cumsum(torch.bincount(user, minlength=self.num_users), 0)
        value = self.beh_idx + 1 if self.shifted else self.beh_idx
        keep = (value >= 1) & (value <= self.num_items)
        span = self.num_items + 1
        keys = torch.unique(user[keep] * span + value[keep])
        owner = torch.div(keys, span, rounding_mode="floor")
        self.avoid_idx = (keys - owner * span).contiguous()
        self.avoid_ptr = torch.zeros(self.num_users + 1, dtype=torch.int64, device=self.device)
        self.avoid_ptr[1:] = torch.cumsum(torch.bincount(owner, minlength=self.num_users), 0)
        self.flag = engine.new_error_flag(self.device)
        self._history = {}

    def history(self, mode):
        """(ptr [num_users + 1], idx) on the device: row u holds the ascending, duplicate-free ``id + 1`` of
        ``row[0, max(0, n - cut))`` with cut = 3 / 2 / 1 for 'train' / 'valid' / 'test' — every interaction the model
        may see for that mode (not only the last ``max_seq_len``), the exclude lists of full-catalogue evaluation.
        Always the items themselves, whatever ``shifted``; built once per mode."""
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}")
        if mode not in self._history:
            cut = 3 - MODES.index(mode)
            n = self.beh_ptr[1:] - self.beh_ptr[:-1]
            user = torch.repeat_interleave(torch.arange(self.num_users, device=self.device), n)
            at = torch.arange(self.beh_idx.numel(), device=self.device) - self.beh_ptr[:-1][user]
            value = self.beh_idx + 1
            keep = (at < (n - cut)[user]) & (value >= 1) & (value <= self.num_items)
            span = self.num_items + 1
            keys = torch.unique(user[keep] * span + value[keep])
            owner = torch.div(keys, span, rounding_mode="floor")
            ptr = torch.zeros(self.num_users + 1, dtype=torch.int64, device=self.device)
            ptr[1:] = torch.cumsum(torch.bincount(owner, minlength=self.num_users), 0)
            self._history[mode] = (ptr, (keys - owner * span).contiguous())
        return self._history[mode]

    @classmethod
    def from_frame(cls, df, num_items, max_seq_len, device, seed=0, shifted=False):
        """From a frame with one ``behaviors`` list per row (``S3RecDataPipeline.preprocess`` / ``split``): user k is
        row k, as ``S3RecDataset.__getitem__`` indexes it."""
        import numpy as np
        rows = df['behaviors'].values
        counts = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
        items = np.fromiter((v for r in rows for v in r), dtype=np.int64, count=int(counts.sum()))
        users = np.repeat(np.arange(len(rows), dtype=np.int64), counts)
        if torch.device(device).type != "cuda":
            raise engine.EngineError("S3RecSequences runs on the GPU only (csrc/s3rec_batches.hip); the host path is "
                                     "DataLoader(S3RecDataset)")
        return cls(torch.from_numpy(users).to(device), torch.from_numpy(items).to(device), len(rows), num_items,
                   max_seq_len, seed=seed, shifted=shifted)

    def __len__(self):
        return self.num_users

    def draw(self, mode, epoch, users=None, n_neg=None, seed=None):
        """(X, pos_items, neg_items) for 'train' / 'valid', (X, pos_item, neg_items) for 'test' — int64 tensors, the
        rows of ``users`` (default: every user, in order) in epoch ``epoch`` under ``seed`` (default: the store's)."""
        if users is None:
            users = torch.arange(self.num_users, device=self.device)
        return engine.s3rec_batches(self.beh_ptr, self.beh_idx, self.avoid_ptr, self.avoid_idx, self.num_items,
                                    users.contiguous(), self.max_seq_len, mode, self.seed if seed is None else seed,
                                    epoch, n_neg=n_neg, err_flag=self.flag)

    def check(self):
        engine.raise_on_flag(self.flag, "S3RecSequences")


class S3RecBatchLoader:
    """Iterable of batch dicts with the reference DataLoader's keys (``user_id``, ``X``, ``pos_items`` / ``pos_item``,
    ``neg_items``), tensors already on the device — the fast path replacing ``DataLoader(S3RecDataset)``.  Every
    ``iter()`` is a new epoch: the user order comes from ``torch.randperm`` under the loader's own generator seeded by
    (seed, epoch) (the test loader never shuffles), the whole epoch is drawn in one launch and sliced."""

    def __init__(self, store: S3RecSequences, mode="train", batch_size=32, shuffle=False, seed=0, n_neg=99):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}")
        self.store, self.mode, self.batch_size = store, mode, int(batch_size)
        self.shuffle = bool(shuffle) and mode != "test"
        self.seed, self.n_neg, self.epoch_no = int(seed), int(n_neg), 0
        self._gen = torch.Generator()

    def __len__(self):
        return (len(self.store) + self.batch_size - 1) // self.batch_size

    def order(self, epoch):
        """The user order of epoch ``epoch``."""
        n = len(self.store)
        if not self.shuffle:
            return torch.arange(n, device=self.store.device)
        self._gen.manual_seed((self.seed * 0x9E3779B97F4A7C15 + epoch) & (2**63 - 1))
        return torch.randperm(n, generator=self._gen).to(self.store.device)

    def __iter__(self):
        epoch = self.epoch_no
        self.epoch_no += 1
        users = self.order(epoch)
        test = self.mode == "test"
        X, pos, neg = self.store.draw(self.mode, epoch, users, n_neg=self.n_neg if test else None, seed=self.seed)
        for lo in range(0, users.numel(), self.batch_size):
            s = slice(lo, lo + self.batch_size)
            yield {"user_id": users[s], "X": X[s], "pos_item" if test else "pos_items": pos[s], "neg_items": neg[s]}
        self.store.check()
