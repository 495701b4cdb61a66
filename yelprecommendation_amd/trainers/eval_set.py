"""Evaluation sets on the device: the reference's eval frames (indexed by user_id, list columns 'pos_items' and
'mask_items', mf_data_pipeline.py:49-50) as CSR tensors, built once per frame and shared by the trainers that
score whole user sets (MF, NGCF, DCN)."""
import numpy as np
import torch

from .. import engine


def _lists_to_csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=ptr[1:])
    idx = np.fromiter((x for l in lists for x in l), dtype=np.int64, count=int(ptr[-1]))
    return ptr, idx


def eval_csr(users, pos, masks, device):
    """(pos lists, users, mask_ptr, mask_idx, pos_ptr, pos_idx) of an evaluation set on the device: the held-out
    lists in their original order (the metrics depend on it) and the mask lists as CSR."""
    mask_ptr, mask_idx = _lists_to_csr(masks)
    pos_ptr, pos_idx = _lists_to_csr(pos)
    return (pos, torch.from_numpy(users).to(device), torch.from_numpy(mask_ptr).to(device),
            torch.from_numpy(mask_idx).to(device), torch.from_numpy(pos_ptr).to(device),
            torch.from_numpy(pos_idx).to(device))


class EvalSets:
    """The eval_csr() tuples of one trainer's evaluation frames, cached by frame."""

    def __init__(self, device):
        self.device = device
        self._cache = {}

    def eval_set(self, eval_data, limit=None, sort_masks=False, keep=None):
        """(eval_data,) + eval_csr(...) of the first ``limit`` rows (all when None).  ``keep``: a predicate over the
        user-id array, the rows to retain (a rank's own users).  A frame is always asked for with the same
        ``sort_masks`` / ``keep`` by its trainer, so (frame, limit) is the key; the cached tuple holds the frame
        itself, so its id() is never reused while cached."""
        key = (id(eval_data), limit)
        if key not in self._cache:
            part = eval_data if limit is None else eval_data[:limit]
            users = np.asarray(part.index.values, dtype=np.int64)
            pos = [list(x) for x in part['pos_items']]
            # sort_masks: ascending ids inside every mask list, what the fused evaluation kernel walks with a cursor
            # (sorted once here instead of on the device at every evaluate())
            masks = [sorted(x) if sort_masks else list(x) for x in part['mask_items']]
            if keep is not None:
                rows = np.flatnonzero(keep(users))
                users, pos, masks = users[rows], [pos[k] for k in rows], [masks[k] for k in rows]
            self._cache[key] = (eval_data,) + eval_csr(users, pos, masks, self.device)
        return self._cache[key]


def top_k_of_scores(pred, mask_items, top_n):
    """reference mf_trainer.py:163-178 / ngcf_trainer.py:167-182 for ONE user's score vector (kept for callers
    that score users one at a time): the ``top_n`` best item ids as a NumPy array, ``mask_items`` excluded."""
    dev = pred.device
    mask = torch.as_tensor(np.asarray(mask_items, dtype=np.int64), device=dev)
    ptr = torch.tensor([0, mask.numel()], dtype=torch.int64, device=dev)
    top = engine.topk_masked(pred.detach().reshape(1, -1).contiguous(), ptr, mask, top_n)
    return top[0].cpu().numpy()
