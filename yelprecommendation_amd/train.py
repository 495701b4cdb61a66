"""Entry point — counterpart of reference train.py:74-204 for the models on the accelerated path
(MF, NGCF, CDAE, DCN, S3Rec fine-tuning).  hydra / wandb are not required: the config is ``configs/train_config.yaml`` in
the reference's layout (or the built-in defaults) plus ``key=value`` overrides.

    python -m yelprecommendation_amd.train model_name=MF data_dir=data/ epochs=5 batch_size=4096
    python -m yelprecommendation_amd.train model_name=MF synthetic=yelp2018 fast_loader=true
    python -m yelprecommendation_amd.train model_name=DCN synthetic=yelp2018 fast_loader=true hidden_dims=[64,32]
    python -m yelprecommendation_amd.train model_name=S3Rec synthetic=yelp2018 fast_loader=true batch_size=256
    python -m yelprecommendation_amd.train model_name=S3Rec synthetic=yelp2018 fast_loader=true full_eval=true
    python -m yelprecommendation_amd.train model_name=NGCF synthetic=yelp2018 fast_loader=true full_eval=true

Call order is the reference's: pipeline.preprocess() -> split() -> datasets -> set_seed() ->
DataLoaders -> trainer.run() -> load_best_model() -> evaluate(test).
"""
import logging
import sys

import pandas as pd
from torch.utils.data import DataLoader

from .utils import Config, load_config, logger, make_config, set_seed


def _parse_overrides(argv):
    out = {}
    for a in argv:
        if "=" not in a:
            raise SystemExit(f"expected key=value, got {a!r}")
        k, v = a.split("=", 1)
        if v.startswith("[") and v.endswith("]"):          # list values such as hidden_dims=[64,32]
            out[k] = [_parse_scalar(x.strip()) for x in v[1:-1].split(",") if x.strip()]
            continue
        out[k] = _parse_scalar(v)
    return out


def _parse_scalar(v):
    for cast in (int, float):
        try:
            return cast(v)
        except ValueError:
            continue
    if v.lower() in ("true", "false"):
        return v.lower() == "true"
    return v


def build(cfg):
    """reference train.py:134-192: pipeline, split, datasets, model_info."""
    from .data.datasets.mf_data_pipeline import MFDataPipeline
    from .data.datasets.mf_dataset import MFDataset
    from .data.datasets.ngcf_data_pipeline import NGCFDataPipeline
    args = Config()
    if cfg.model_name == 'MF':
        pipe = MFDataPipeline(cfg)
    elif cfg.model_name == 'NGCF':
        pipe = NGCFDataPipeline(cfg)
    elif cfg.model_name == 'CDAE':
        from .data.datasets.cdae_data_pipeline import CDAEDataPipeline
        pipe = CDAEDataPipeline(cfg)
    elif cfg.model_name == 'DCN':
        from .data.datasets.dcn_data_pipeline import DCNDataPipeline
        pipe = DCNDataPipeline(cfg)
    elif cfg.model_name == 'S3Rec':
        from .data.datasets.s3rec_data_pipeline import S3RecDataPipeline
        pipe = S3RecDataPipeline(cfg)
    else:
        raise ValueError(f"model '{cfg.model_name}' is not on the accelerated path (MF, NGCF, CDAE, DCN, S3Rec)")
    synthetic = cfg.get("synthetic")
    if synthetic:
        from .data.synthetic import make_frame
        if synthetic == "yelp2018":
            import torch
            if str(cfg.device).lower() == "cuda" and torch.cuda.is_available():
                # same generative model drawn on the GPU (seconds instead of ~30 s of NumPy)
                from .data.synthetic import make_interactions_torch
                u, i = make_interactions_torch(mean_items=47.0, min_item_degree=5, device="cuda")
                r = torch.randint(1, 6, u.shape, device=u.device, generator=torch.Generator(device=u.device).manual_seed(1234))
                df = pd.DataFrame({"user_id": u.cpu().numpy(), "business_id": i.cpu().numpy(), "rating": r.cpu().numpy()})
            else:
                df = make_frame(mean_items=47.0, min_item_degree=5)
        else:
            nu, ni, mean = (float(x) for x in str(synthetic).split("x"))
            df = make_frame(int(nu), int(ni), mean)
        pipe._load_df = lambda: df
        if cfg.model_name in ('DCN', 'S3Rec'):
            # the attributes of the synthetic catalogue, in the schema of yelp_item2attributes.json
            from .data.synthetic import make_item_attributes
            attrs = make_item_attributes(int(df.business_id.max()) + 1)
            attr_frame = pd.DataFrame.from_dict({int(k): v for k, v in attrs.items()}, orient='index')
            pipe._read_attributes = lambda: attr_frame.copy()
    args.data_pipeline = pipe
    if cfg.model_name == 'CDAE' and cfg.get("fast_loader"):
        # sparse device-side store instead of the dense pivot + four dense masks per user
        import torch
        from .data.cdae_batches import CDAEInteractions
        raw = pipe._load_df()
        nu, ni = int(raw.user_id.max()) + 1, int(raw.business_id.max()) + 1
        args.cdae_data = CDAEInteractions.from_interactions(
            torch.from_numpy(raw.user_id.values.astype('int64')), torch.from_numpy(raw.business_id.values.astype('int64')),
            nu, ni, seed=cfg.seed, device=cfg.device)
        args.model_info = {'num_items': ni, 'num_users': nu}
        return args
    df = pipe.preprocess()
    if cfg.model_name == 'CDAE':
        from .data.datasets.cdae_dataset import CDAEDataset
        train_data, valid_data, test_data = pipe.split(df)
        args.train_dataset = CDAEDataset(train_data, 'train', neg_times=cfg.neg_times)
        args.valid_dataset = CDAEDataset(valid_data, 'valid', neg_times=cfg.neg_times)
        args.test_dataset = CDAEDataset(test_data, 'test')
        args.model_info = {'num_items': len(df.columns) - 1, 'num_users': len(train_data)}
    elif cfg.model_name == 'S3Rec':
        # reference train.py:178-184
        from .data.datasets.s3rec_dataset import S3RecDataset
        train_data, valid_data, test_data = pipe.split(df)
        attrs = (pipe.item2attributes, pipe.attributes_count)
        args.train_dataset = S3RecDataset(train_data, *attrs, num_items=pipe.num_items)
        args.valid_dataset = S3RecDataset(valid_data, *attrs, num_items=pipe.num_items)
        args.test_dataset = S3RecDataset(test_data, *attrs, num_items=pipe.num_items, train=False)
        args.model_info = {'num_items': pipe.num_items, 'num_users': pipe.num_users}
    else:
        train_data, valid_data, valid_eval_data, test_eval_data = pipe.split(df)
        args.train_dataset = MFDataset(train_data, num_items=pipe.num_items)
        args.valid_dataset = MFDataset(valid_data, num_items=pipe.num_items)
        args.valid_eval_data, args.test_eval_data = valid_eval_data, test_eval_data
        args.model_info = {'num_items': pipe.num_items, 'num_users': pipe.num_users}
        if cfg.model_name == 'DCN':
            args.model_info.update(item2attributes=pipe.item2attributes, attributes_count=pipe.attributes_count,
                                   cat_ids=pipe.cat_ids, sc_ids=pipe.sc_ids)
    return args


CDAE_LIST_HIDDEN = (16, 32, 64, 128, 256, 512, 1024)
CDAE_PLAIN_LIST_HIDDEN = (16, 32, 64, 128)      # negative_sampling=false: the catalogue sweep's widths


def cdae_takes_list_batches(cfg, num_items):
    """CDAE batches as lists straight from the per-user CSR (no dense rows or masks)?  When the fused step and the
    fused evaluation can take them: Adam / AdamW, a hidden size the kernels are built for (NS-BCE: the sweep grid's
    powers of two; plain BCE, ``negative_sampling=false``: the four widths of the catalogue sweep — wider models keep
    dense batches there), a top-n the fused evaluation has at that width (n <= 16 from 128 up)."""
    from .engine import fused_eval_supports
    widths = CDAE_LIST_HIDDEN if cfg.negative_sampling else CDAE_PLAIN_LIST_HIDDEN
    return bool(cfg.get("list_batches", True)) and bool(cfg.get("fused_step", True)) \
        and cfg.optimizer.lower() in ("adam", "adamw") and cfg.hidden_size in widths \
        and bool(fused_eval_supports(cfg.top_n, cfg.hidden_size)) and num_items <= 163840


def train(cfg, args):
    """reference train.py:74-115."""
    from .trainers.mf_trainer import MFTrainer
    from .trainers.ngcf_trainer import NGCFTrainer
    if cfg.model_name == 'S3Rec':
        return _train_s3rec(cfg, args)
    if cfg.model_name == 'NGCF' and cfg.get("deterministic", False):
        from .ngcf_step import DETERMINISTIC_NEEDS, deterministic_available
        if not deterministic_available(cfg):                   # refused before training starts, never run unordered
            raise NotImplementedError(DETERMINISTIC_NEEDS)
    if cfg.get("fast_loader") and cfg.model_name in ('MF', 'NGCF', 'DCN'):
        # device-side epoch sampler instead of DataLoader(MFDataset): same distribution, own RNG
        from .data.triplets import EpochLoader
        import torch
        dev = torch.device(cfg.device)
        nu = args.model_info['num_users']
        train_dataloader = EpochLoader(args.train_dataset.to_sampler(dev, nu, seed=cfg.seed), cfg.batch_size, cfg.shuffle)
        valid_dataloader = EpochLoader(args.valid_dataset.to_sampler(dev, nu, seed=cfg.seed + 1), cfg.batch_size, cfg.shuffle)
    elif not (cfg.get("fast_loader") and cfg.model_name == 'CDAE'):
        train_dataloader = DataLoader(args.train_dataset, batch_size=cfg.batch_size, shuffle=cfg.shuffle)
        valid_dataloader = DataLoader(args.valid_dataset, batch_size=cfg.batch_size, shuffle=cfg.shuffle)
    if cfg.model_name == 'CDAE':
        from .trainers.cdae_trainer import CDAETrainer
        if cfg.get("deterministic", False) and not (cfg.get("fast_loader") and
                                                    cdae_takes_list_batches(cfg, args.cdae_data.num_items)):
            from .cdae_step import DETERMINISTIC_NEEDS       # refused before training starts, never run unordered
            raise NotImplementedError(DETERMINISTIC_NEEDS)
        if cfg.get("fast_loader"):
            from .data.cdae_batches import CDAEBatchLoader
            as_lists = cdae_takes_list_batches(cfg, args.cdae_data.num_items)
            # the test metrics over list batches are computed for all users at once (CDAETrainer._scored_by_lists), so
            # the rows per evaluation batch do not enter the result: fewer, larger batches (7.1 -> 5.4 ms at Yelp2018 size)
            rows = lambda mode: max(cfg.batch_size, int(cfg.get("eval_batch_size", 4096))) if as_lists and mode == 'test' \
                else cfg.batch_size
            mk = lambda mode, seed: CDAEBatchLoader(args.cdae_data, mode, rows(mode), cfg.neg_times,
                                                    shuffle=cfg.shuffle and mode != 'test', seed=seed, lists=as_lists,
                                                    dropout=cfg.corruption_level,
                                                    negative_sampling=bool(cfg.negative_sampling))
            train_dataloader, valid_dataloader, test_dataloader = mk('train', cfg.seed), mk('valid', cfg.seed + 1), mk('test', 0)
        else:
            test_dataloader = DataLoader(args.test_dataset, batch_size=cfg.batch_size)
        trainer = CDAETrainer(cfg, args.model_info['num_items'], args.model_info['num_users'])
        trainer.run(train_dataloader, valid_dataloader)
        trainer.load_best_model()
        return trainer, trainer.evaluate(test_dataloader)
    if cfg.model_name == 'MF':
        trainer = MFTrainer(cfg, args.model_info['num_items'], args.model_info['num_users'])
    elif cfg.model_name == 'DCN':
        from .trainers.dcn_trainer import DCNTrainer
        info = args.model_info
        trainer = DCNTrainer(cfg, info['num_items'], info['num_users'], info['item2attributes'],
                             info['attributes_count'], cat_ids=info['cat_ids'], sc_ids=info['sc_ids'])
    else:
        trainer = NGCFTrainer(cfg, args.model_info['num_items'], args.model_info['num_users'],
                              args.data_pipeline.laplacian_matrix)
    trainer.run(train_dataloader, valid_dataloader, args.valid_eval_data)
    trainer.load_best_model()
    if not (cfg.get("rank_eval") and cfg.model_name in ('MF', 'NGCF')):
        return trainer, trainer.evaluate(args.test_eval_data, 'test')
    # rank_eval: every cutoff of eval_ks from ONE rank sweep, with HR, MRR and AUC (logged); the return value stays the
    # four figures at top_n
    ks = cfg.get("eval_ks") or [cfg.top_n]
    ks = [int(k) for k in (ks if isinstance(ks, (list, tuple)) else [ks])]
    if cfg.model_name == 'NGCF' and not cfg.get("full_eval"):
        # evaluate() is the reference's 100-row sample and does not look at rank_eval
        result = trainer.evaluate(args.test_eval_data, 'test')
        logger.info(f"[Trainer] full_eval is off: the figures above are the 100-row sample; rank evaluation of ALL "
                    f"rows of the test frame follows, eval_ks={ks}")
        trainer.evaluate_ranks(args.test_eval_data, ks=ks, mode='test')
        return trainer, result
    logger.info(f"[Trainer] rank evaluation of the test frame, eval_ks={ks}")
    top_n = int(cfg.top_n)
    res = trainer.evaluate_ranks(args.test_eval_data, ks=list(dict.fromkeys(ks + [top_n])), mode='test')
    result = tuple(res[top_n][:4])
    trainer._log_test(*result)
    return trainer, result


def _train_s3rec(cfg, args):
    """reference train.py:104-115: with pretrain=true the pre-training of :105-109 on the train loader first (its
    best model is what S3RecTrainer then picks up through load_pretrain), then fine-tuning."""
    if cfg.get("pretrain") and str(cfg.device).lower() != "cuda":
        raise NotImplementedError(f"S3Rec pre-training is not built for the {cfg.device} device (pretrain=true): the "
                                  "kernels run on the GPU only")
    from .trainers.s3rec_trainer import S3RecPreTrainer, S3RecTrainer
    if cfg.get("fast_loader"):
        # device-side batch builder instead of DataLoader(S3RecDataset): same law, own RNG
        import torch
        from .data.s3rec_batches import S3RecBatchLoader
        store = args.train_dataset.to_sequences(torch.device(cfg.device), cfg.max_seq_len, seed=cfg.seed)
        mk = lambda mode, seed: S3RecBatchLoader(store, mode, cfg.batch_size, shuffle=cfg.shuffle, seed=seed)
        train_dataloader, valid_dataloader, test_dataloader = mk('train', cfg.seed), mk('valid', cfg.seed + 1), mk('test', 0)
    else:
        train_dataloader = DataLoader(args.train_dataset, batch_size=cfg.batch_size, shuffle=cfg.shuffle)
        valid_dataloader = DataLoader(args.valid_dataset, batch_size=cfg.batch_size, shuffle=cfg.shuffle)
        test_dataloader = DataLoader(args.test_dataset, batch_size=cfg.batch_size)
    if cfg.get("pretrain"):
        pretrainer = S3RecPreTrainer(cfg, args.model_info['num_items'], args.data_pipeline.item2attributes,
                                     args.data_pipeline.attributes_count)
        pretrainer.pretrain(train_dataloader)
        pretrainer.load_best_model()
    trainer = S3RecTrainer(cfg, args.model_info['num_items'], args.data_pipeline.item2attributes,
                           args.data_pipeline.attributes_count)
    trainer.run(train_dataloader, valid_dataloader)
    trainer.load_best_model()
    result = trainer.evaluate(test_dataloader)
    if cfg.get("full_eval"):
        # the held-out item against the whole catalogue, the user's earlier items left out (logged; the return value
        # stays the reference's sampled protocol)
        import torch
        if not cfg.get("fast_loader"):
            store = args.test_dataset.to_sequences(torch.device(cfg.device), cfg.max_seq_len, seed=cfg.seed)
        trainer.evaluate_full(test_dataloader, history=store.history('test'))
    return trainer, result


def run(cfg, args):
    """reference train.py:56-60 (wandb init/finish omitted)."""
    set_seed(cfg.seed)
    return train(cfg, args)


def _init_distributed():
    """One process per GPU under ``python -m torch.distributed.run`` (MF only: the interaction
    matrix is then sharded by user, see trainers/mf_trainer.py); a plain launch stays single-GPU."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return False
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)              # RCCL over xGMI
    return True


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    distributed = _init_distributed()
    over = _parse_overrides(sys.argv[1:] if argv is None else argv)
    path = over.pop("config", None)
    model_name = over.pop("model_name", "MF")
    cfg = load_config(path, model_name=model_name, **over) if path else make_config(model_name, **over)
    args = build(cfg)
    trainer, metrics = run(cfg, args)
    logger.info(f"test precision/recall/map/ndcg @{cfg.top_n}: {metrics}")
    if distributed:
        import torch.distributed as dist
        dist.destroy_process_group()
    return metrics


if __name__ == '__main__':
    main()
