"""The DCN entry point on the host: ``train.build()`` for the DCN pipeline with the synthetic data forms (the
attribute table is generated next to the interactions), and the packing of the cross-network parameters and
gradients into [L, F] blocks that the head kernel reads."""
import numpy as np
import pytest
import torch


@pytest.mark.parametrize("synthetic", ["60x40x5", "300x200x12"])
def test_build_dcn_with_synthetic_frames(synthetic):
    from yelprecommendation_amd.train import build
    from yelprecommendation_amd.utils import make_config
    args = build(make_config("DCN", device="cpu", synthetic=synthetic))
    info = args.model_info
    ni = info["num_items"]
    cats, sc = info["cat_ids"].numpy(), info["sc_ids"].numpy()
    assert cats.shape[0] == ni and sc.shape == (ni,) and cats.dtype == np.int32
    n_cat, n_sc = info["attributes_count"]
    assert cats.min() >= 0 and cats.max() == n_cat and (cats == 0).any()     # shifted ids, slot 0 = padding
    assert sc.min() >= 0 and sc.max() == n_sc - 1
    assert info["item2attributes"][0]["categories"] == cats[0].tolist()
    assert len(args.train_dataset) > 0 and len(args.valid_eval_data) > 0


def test_as_block_only_for_slices_of_one_storage():
    from yelprecommendation_amd.models.dcn import _as_block
    flat = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    blk = _as_block([flat[0], flat[1], flat[2]])
    assert blk is not None and torch.equal(blk, flat)
    assert _as_block([flat[0], flat[2]]) is None                      # not consecutive
    assert _as_block([torch.zeros(4), torch.zeros(4)]) is None        # separate storages, whatever their addresses
    big = torch.zeros(16)
    assert _as_block([big[0:4], big[4:8]]) is not None and _as_block([big[4:8], big[0:4]]) is None
    assert _as_block([flat[0], None]) is None


def test_cross_blocks_are_the_parameters_and_keep_gradients():
    from yelprecommendation_amd.models.dcn import DCN
    from yelprecommendation_amd.utils import make_config
    cfg = make_config("DCN", device="cpu", embed_size=16, hidden_dims=[64], cross_orders=3)
    torch.manual_seed(0)
    m = DCN(cfg, 10, 12, [4, 3])
    w, b = m._cross_packed()
    for l in range(3):
        assert w[l].data_ptr() == m.cross_weights[l].data_ptr() and b[l].data_ptr() == m.cross_bias[l].data_ptr()
    before = [p.detach().clone() for p in m.cross_weights]
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, assign=True)     # fresh, separate tensors
    w, _ = m._cross_packed()
    for l in range(3):
        assert torch.equal(w[l], before[l]) and w[l].data_ptr() == m.cross_weights[l].data_ptr()
    # per-row gradients (what autograd leaves) are packed with their values kept
    for l, p in enumerate(m.cross_weights):
        p.grad = torch.full_like(p, float(l + 1))
    gw, gb = m._cross_grads()
    assert torch.equal(gw[:, 0], torch.tensor([1.0, 2.0, 3.0])) and float(gb.abs().sum()) == 0.0
    for l in range(3):
        assert m.cross_weights[l].grad.data_ptr() == gw[l].data_ptr()
