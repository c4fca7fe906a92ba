"""Training driver with the reference's CLI surface (src/train.py:62-73) around the HIP hot path.

    python -m mau_amd.train --device gpu --model-type unet --no-temporal-embeddings --epochs 1 --steps-per-epoch 20
    python -m mau_amd.train --device gpu --model-type unet --no-temporal-embeddings --epochs 1 --processed-dir data/processed
    python -m mau_amd.train --device gpu --model-type unet --no-temporal-embeddings --epochs 1 --ssim-gradient

The reference wraps the step in Optuna trials, wandb logging and a dataset that is not shipped
(SURVEY D9); none of that is on the hot path.  This driver keeps: the flags, the study-name suffix
rule (:79-87), seeding (:104), model construction (:194-207), optimizer / loss selection
(:209-225), the inner step (:243-256), ``validate()`` (:20-60: eval-mode pass over a held-out split,
sample-weighted means of the criterion's total and of every term of ``compute_all_loss``, all from one launch per batch), the
running-loss step log (:230-277), best-VALIDATION checkpointing in the exact ``.pth`` layout (:303-319) -- on the ``train/`` and
``val/`` folders of a processed dataset (``--processed-dir``: the loaders of :172-192 through ``data.DeviceLoader``), or without one on
synthetic batches with the loader's tuple layout (src/dataset.py:87-108).
Single process (the train step is one hipGraph replay, ``train_graph.GraphedTrainStep``), or data
parallel under ``torch.distributed.run`` (RCCL; eager step with overlapped collectives).
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch
import typer

from . import compute_loss_l1_grad_ssim, compute_loss_l1_grad_ssim_trained, compute_loss_mse, compute_loss_mse_gradient
from . import data as data_
from .checkpoint import build_hyperparameters, save_checkpoint
from .config import CONFIG
from .functional import typer_device
from .dist import GradSync, init_process_group_from_env
from .losses import ALL_LOSS_TERMS, TERM_MSE_GRADIENT_TOTAL, loss_terms
from .metrics import RunningLoss
from .model import _DTYPES, UrbanPredictor
from .optim import SGD, Adam, AdamW, _PackOptimizer
from .train_graph import GraphedTrainStep

app = typer.Typer(add_completion=False)


def synthetic_batch(batch_size: int, device, gen: torch.Generator):
    """(inputs, metadatas, temp_series_padded, temp_series_lengths, t1_dates, t2_dates, targets), src/dataset.py:87-108."""
    ds = CONFIG.dataset
    e = ds.image_shape_edge
    mk = lambda *s: torch.randn(*s, generator=gen).to(device)
    n_meta = ds.nb_metadata_features
    return (mk(batch_size, ds.nb_input_channels, e, e), mk(batch_size, n_meta - 4 if n_meta >= 8 else n_meta),
            mk(batch_size, 24), torch.full((batch_size,), 24), mk(batch_size, 2), mk(batch_size, 2),
            mk(batch_size, len(ds.target_channels), e, e))


def _checked(loader):
    """The loader's batches, after a look at the packed input: its channel count must be the one the network is built for."""
    class _Checked:
        def __len__(self):
            return len(loader)

        def __iter__(self):
            want = CONFIG.dataset.nb_input_channels
            for batch in loader:
                if batch[0].C != want:
                    raise ValueError(f"the tiles of {loader.loader.dataset.data_dir} have {batch[0].C} input channels, the configuration "
                                     f"(dataset.nb_input_channels) builds the network for {want}")
                yield batch
    return _Checked()


def validate(model: torch.nn.Module, loader, criterion, watchdog=None):
    """Loss on the validation set (src/train.py:20-60): eval mode, no_grad, every batch weighted by its sample count; a batch that
    is refused with ValueError (a tile too small for SSIM) is skipped and does not count; the model is put back into training mode.
    Returns (mean of the criterion's ``total``, {key: mean} over the five keys of ``compute_all_loss``) -- ``(inf, {})`` when no
    batch counted.  All terms of a batch come from ONE launch (``mau_loss_terms``) and for the three criteria of this driver the
    batch ``total`` is one of them (mse: terms[0], mse-gradient: terms[6], l1-gradient-ssim: terms[7]); any other callable is
    called as well.  The sums stay on the device and are read back once after the loop.  With a ``watchdog`` the stream is
    synchronised once per batch before ``kick()``: the kick means "the GPU was there"."""
    n_meta = CONFIG.dataset.nb_metadata_features
    own = {compute_loss_mse: 0, compute_loss_mse_gradient: TERM_MSE_GRADIENT_TOTAL, compute_loss_l1_grad_ssim: ALL_LOSS_TERMS["total"],
           compute_loss_l1_grad_ssim_trained: ALL_LOSS_TERMS["total"]}
    idx = own.get(criterion)
    model.eval()
    acc = other = None
    num = 0
    with torch.no_grad():
        for inputs, metadata, temp_series, _lengths, t1, t2, targets in loader:
            metadata_full = torch.cat([metadata, t1, t2], dim=1) if n_meta >= 8 else metadata
            outputs = model(inputs, temp_series, metadata_full)
            try:
                batch_loss = criterion(outputs, targets)["total"] if idx is None else True
                if acc is None:
                    acc = torch.zeros(8, dtype=torch.float64, device=outputs.device)
                loss_terms(outputs, targets, acc=acc)                                       # src/train.py:44-48, kept on the device
                if batch_loss is not None:
                    if idx is None:                                                         # src/train.py:42: .item() * len(batch)
                        w = batch_loss.detach().double() * len(targets)
                        other = w if other is None else other + w
                    num += len(targets)
                    if watchdog is not None:
                        torch.cuda.current_stream().synchronize()
                        watchdog.kick()
            except ValueError as e:
                typer.echo(f"Skipping batch in validation due to error: {e}")
                continue
    model.train()
    if num == 0:
        return float("inf"), {}
    sums = acc.cpu().tolist()                                                               # the pass's one read-back
    total = sums[idx] if idx is not None else float(other.cpu())
    return total / num, {k: sums[i] / num for k, i in ALL_LOSS_TERMS.items()}


@app.command()
def main(device: str = "", wandblog: bool = False, n_trials: int = 1, force_study_name: bool = False,
         temporal_embeddings: bool = True, metadata_embeddings: bool = True, study_name: str = "urban-predictor",
         model_type: str = "unet++", jobid: str = "", epochs: Optional[int] = None, steps_per_epoch: int = 20,
         precision: str = "bf16", val_batches: int = 2, graph: bool = True, processed_dir: Optional[str] = None,
         num_workers: int = 0, batch_size: Optional[int] = None, ssim_gradient: bool = False):
    """The reference's CLI (src/train.py:62-73) + --epochs / --steps-per-epoch / --precision / --val-batches / --no-graph /
    --processed-dir (train on <dir>/train, validate on <dir>/val) / --num-workers / --batch-size / --ssim-gradient (with the
    l1-gradient-ssim loss: train on the SSIM term too, which the reference detaches)."""
    return run(device, wandblog, n_trials, force_study_name, temporal_embeddings, metadata_embeddings, study_name, model_type,
               jobid, epochs, steps_per_epoch, precision, val_batches, graph, processed_dir=processed_dir, num_workers=num_workers,
               batch_size=batch_size, ssim_gradient=ssim_gradient)["best"]


def run(device: str = "", wandblog: bool = False, n_trials: int = 1, force_study_name: bool = False,
        temporal_embeddings: bool = True, metadata_embeddings: bool = True, study_name: str = "urban-predictor",
        model_type: str = "unet++", jobid: str = "", epochs: Optional[int] = None, steps_per_epoch: int = 20,
        precision: str = "bf16", val_batches: int = 2, graph: bool = True, force_dist: bool = False,
        processed_dir: Optional[str] = None, num_workers: int = 0, batch_size: Optional[int] = None, ssim_gradient: bool = False):
    """Body of the CLI as a function; returns {'best' (validation loss), 'model', 'optimizer', 'checkpoint_path', 'history',
    'val_terms' (per epoch, the second value of ``validate``), 'step'}.
    ``force_dist``: take the data-parallel path (SyncBN + GradSync over the default process group) even with one rank -- the
    one-GPU rehearsal of the RCCL code path (tests/test_gpu_dist_rehearsal.py).
    ``processed_dir``: the folder the reference's ``process_and_save_subset`` wrote; the loaders of src/train.py:172-192 over
    ``<dir>/train`` (shuffled, RandomFlip) and ``<dir>/val``.  An epoch is then ONE PASS over the train loader and validation runs
    over the whole ``val/`` split: ``steps_per_epoch`` and ``val_batches`` are ignored.  The ragged last batch is not dropped (nor is
    a batch whose time series is padded to another length): the graph is captured for the first full batch's shapes, a batch of
    other shapes takes the eager step.  ``batch_size`` overrides the yaml value.  One process only.
    ``ssim_gradient``: with ``training.loss == "l1-gradient-ssim"`` the criterion is ``compute_loss_l1_grad_ssim_trained`` (the SSIM
    term reaches the weights) and the checkpoint's hyperparameters say ``ssim_gradient: True``; any other loss has no SSIM term and
    is refused.  Off, everything is as the reference has it, the checkpoint's keys included."""
    assert model_type in ["unet", "unet++"], "model_type must be 'unet' or 'unet++'"          # src/train.py:78
    if not force_study_name:                                                                  # src/train.py:79-87
        study_name += "-emb" if temporal_embeddings and metadata_embeddings else "-tempemb" if temporal_embeddings \
            else "-metaemb" if metadata_embeddings else "-noemb"
    typer_device(device)
    if ssim_gradient and CONFIG.training.loss != "l1-gradient-ssim":                          # before anything touches the GPU
        raise ValueError(f"--ssim-gradient needs training.loss 'l1-gradient-ssim'; the loss '{CONFIG.training.loss}' has no SSIM term")
    if processed_dir is not None:                    # before anything touches the GPU: a wrong path is the likeliest mistake
        for split in ("train", "val"):
            if not os.path.isdir(os.path.join(processed_dir, split)):
                raise FileNotFoundError(f"Directory for split '{split}' not found at: {os.path.join(processed_dir, split)}")
    rank, local, world = init_process_group_from_env()
    import torch.distributed as dist
    data_parallel = world > 1 or (force_dist and dist.is_available() and dist.is_initialized())
    if processed_dir is not None and data_parallel:
        raise NotImplementedError("processed_dir with more than one rank is out of scope: the validation sums would have to be "
                                  "all-reduced before the checkpoint decision, and no two-GPU box can test that.")
    CONFIG.device = f"cuda:{local}"
    torch.cuda.set_device(local)
    torch.manual_seed(CONFIG.seed)                                                            # src/train.py:104
    cfg = CONFIG.training
    n_meta = CONFIG.dataset.nb_metadata_features
    model = UrbanPredictor(model_type=model_type, spatial_channels=CONFIG.dataset.nb_input_channels,
                           seq_len=CONFIG.dataset.temporal_length, temporal_dim=cfg.temporal_dim, meta_features=n_meta,
                           meta_dim=cfg.meta_dim, lstm_dim=cfg.lstm_hidden, out_channels=len(CONFIG.dataset.target_channels),
                           deep_supervision=False, temporal_embeddings=temporal_embeddings,
                           metadata_embeddings=metadata_embeddings).to(CONFIG.device)              # src/train.py:194-206
    model.set_precision(precision).train()
    # torch.optim's rules; the convolution weights' update + re-pack is one kernel (optim.py)
    if cfg.optimizer == "SGD":                                                                # src/train.py:209-216
        optimizer = SGD(model.parameters(), lr=cfg.learning_rate, momentum=cfg.momentum)
    elif cfg.optimizer == "Adam":
        optimizer = Adam(model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay)
    elif cfg.optimizer == "AdamW":
        optimizer = AdamW(model.parameters(), lr=cfg.learning_rate, weight_decay=cfg.weight_decay)
    else:
        raise NotImplementedError(f"Optimizer {cfg.optimizer} not implemented.")
    if cfg.loss == "mse":                                                                     # src/train.py:218-225
        criterion = compute_loss_mse
    elif cfg.loss == "mse-gradient":
        criterion = compute_loss_mse_gradient
    elif cfg.loss == "l1-gradient-ssim":
        criterion = compute_loss_l1_grad_ssim_trained if ssim_gradient else compute_loss_l1_grad_ssim
    else:
        raise NotImplementedError(f"Loss {cfg.loss} not implemented.")
    sync = watchdog = None
    if data_parallel:
        # Collectives: RCCL called directly on our streams (dist.RcclComm) is the measured path of bench.py, where a supervisor
        # with a fallback stands behind it.  Here nothing does, and two communicators driven from two streams have not yet
        # run between two GPUs: between REAL ranks the training driver goes through ProcessGroupNCCL (its own watchdog, its own
        # timeout) unless MAU_RCCL_DIRECT=1 asks for the direct path -- which then runs under a watchdog of ours.
        direct = (os.environ["MAU_RCCL_DIRECT"] != "0") if "MAU_RCCL_DIRECT" in os.environ else (world == 1)
        model.set_sync_bn(dist.group.WORLD, direct=direct)
        sync = GradSync(model, direct=direct)
        if sync.comm is not None and world > 1:
            from .dist import CollectiveWatchdog
            watchdog = CollectiveWatchdog()
    hyper = build_hyperparameters(cfg, model_type, temporal_embeddings, metadata_embeddings,
                                  CONFIG.dataset.input_channels, CONFIG.dataset.target_channels)
    if ssim_gradient:                                # only then: a checkpoint written without the flag keeps the reference's keys
        hyper["ssim_gradient"] = True
    gen = torch.Generator().manual_seed(CONFIG.seed + rank)
    # held-out synthetic validation split (the reference's val_loader, src/train.py:183-192): drawn once, from its own generator
    vgen = torch.Generator().manual_seed(CONFIG.seed + 7919 + rank)
    bs = int(batch_size) if batch_size is not None else cfg.batch_size
    if processed_dir is None:
        train_loader = None
        val_loader = [synthetic_batch(bs, CONFIG.device, vgen) for _ in range(max(0, val_batches))]
    else:                                                                                     # src/train.py:172-192
        train_loader = _checked(data_.create_dataloader("train", bs, shuffle=True, transform=data_.RandomFlip(CONFIG.seed),
                                                        num_workers=num_workers, processed_dir=processed_dir, device=CONFIG.device,
                                                        dtype=_DTYPES[precision]))
        val_loader = _checked(data_.create_dataloader("val", bs, shuffle=False, transform=None, num_workers=num_workers,
                                                      processed_dir=processed_dir, device=CONFIG.device, dtype=_DTYPES[precision]))
    clip = 5.0 if cfg.gradient_clipping > 0 else 0.0                                            # src/train.py:253-254
    if clip > 0 and isinstance(optimizer, _PackOptimizer):      # norm + coefficient in one launch, the scaling inside the fused update
        optimizer.max_grad_norm, clip = clip, 0.0
    # one GPU: the step (forward, criterion, backward, clip, optimizer) is captured once and replayed (static shapes);
    # data parallel: eager, the RCCL collectives are launched from autograd hooks while backward still runs
    # (MAU_DP_GRAPH=1: the data-parallel step is captured too, collectives included -- train_graph.py)
    dp_graph = sync is not None and os.environ.get("MAU_DP_GRAPH", "0") == "1"
    gstep = GraphedTrainStep(model, optimizer, criterion, clip_grad_norm=clip, grad_sync=sync) if (graph and (sync is None or dp_graph)) else None
    best, step, ckpt_path, history, val_terms = float("inf"), 0, None, [], []
    ema_loss, sma_loss = RunningLoss(mode="ema", ema_alpha=0.98), RunningLoss(mode="sma", window_size=50)   # src/train.py:230-232
    cum_loss = RunningLoss(mode="cumulative")
    log_every = int(CONFIG.get("logging", {}).get("frequency_log", 0) or 0)
    try:
        for epoch in range(epochs if epochs is not None else cfg.epochs):
            model.train()
            total, num = 0.0, 0
            batches = train_loader if train_loader is not None else (synthetic_batch(bs, CONFIG.device, gen) for _ in range(steps_per_epoch))
            for inputs, metadata, temp_series, _lengths, t1, t2, targets in batches:
                metadata_full = torch.cat([metadata, t1, t2], dim=1) if n_meta >= 8 else metadata  # src/train.py:244
                if gstep is not None and gstep.matches(inputs, temp_series, metadata_full, targets) \
                        and (gstep.graph is not None or train_loader is None or len(targets) == bs):
                    batch_loss = gstep(inputs, temp_series, metadata_full, targets)             # src/train.py:245-256 in one replay
                elif gstep is not None:                # a ragged last batch / another padded length: the same step, outside the graph
                    batch_loss = gstep.eager_step(inputs, temp_series, metadata_full, targets)
                else:
                    outputs = model(inputs, temp_series, metadata_full)                         # src/train.py:245
                    batch_loss = criterion(outputs, targets).get("total", None)                 # src/train.py:247-249
                    if sync is not None:
                        sync.begin()
                    batch_loss.backward()
                    if sync is not None:
                        sync.finish()
                    if clip > 0:
                        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)                # src/train.py:253-254
                    optimizer.step()
                    optimizer.zero_grad()
                loss_item = batch_loss.detach().cpu().item()
                total += loss_item * len(targets)                                               # src/train.py:258-260
                if watchdog is not None:
                    watchdog.kick()                                                             # (the read-back above: the step HAS finished)
                num += len(targets)
                step += 1
                ema, sma, cum = ema_loss.update(loss_item), sma_loss.update(loss_item), cum_loss.update(loss_item, n=len(targets))
                if rank == 0 and log_every > 0 and step % log_every == 0:                       # src/train.py:261-277 (the wandb row)
                    typer.echo(f"step {step} | batch loss {loss_item:.6f} | ema {ema:.6f} | sma {sma:.6f} | cumulative {cum:.6f}")
            epoch_loss = total / max(num, 1)
            val_loss, terms = validate(model, val_loader, criterion, watchdog)                  # src/train.py:286
            history.append((epoch_loss, val_loss))
            val_terms.append(terms)
            if rank == 0:
                typer.echo(f"Epoch {epoch + 1} | step {step} | Train Loss: {epoch_loss:.6f} | Val Loss: {val_loss:.6f}")
                if terms:                                                                       # src/train.py:297-299 (val/loss_<key>)
                    typer.echo("    " + " | ".join(f"val/loss_{k}: {v:.6f}" for k, v in terms.items()))
                if val_loss < best:                                                             # src/train.py:303-319
                    best = val_loss
                    name = f"{study_name}_trial_0_best_job{jobid}.pth"
                    ckpt_path = os.path.join(CONFIG.MODELS_DIR, name)
                    with (watchdog.paused() if watchdog is not None else contextlib.nullcontext()):   # slow storage is not a hung collective
                        save_checkpoint(ckpt_path, model, optimizer, epoch=epoch, step=step, loss=best,
                                        hyperparameters=hyper, model_type=model_type, study_name=study_name, trial_id=0,
                                        metadata_input_length=n_meta)
            if watchdog is not None:
                # the other ranks would otherwise sit in the next step's first collective while rank 0 writes: everybody waits HERE, clock
                # stopped, in a barrier of the process group (which has torch's own timeout behind it)
                with watchdog.paused():
                    dist.barrier()
    finally:
        if watchdog is not None:
            watchdog.close()          # also when the loop raises: a caller that handles the exception must not be killed later
    return {"best": best, "model": model, "optimizer": optimizer, "checkpoint_path": ckpt_path, "history": history,
            "val_terms": val_terms, "step": step}


if __name__ == "__main__":
    app()
