"""Training / prediction drivers (the reference's run_tffm.py train() and predict()).

Reference behaviour kept (run_tffm.py:10-90, :213-231):
* ``========  train  ========`` banner; per step ``-- Global Step: %d; Avg loss: %.5f;``;
* ``-m``: ``speed: <ex/s> shuffle_queue: x% example_queue: y%`` per step;
* every ``save_steps``: validation loss ``validation loss at step %d: %.8f`` and
  early stop below ``tolerance`` ("Loss on validation data set is below
  tolerance. Training completed."), checkpoint (CheckpointSaverHook); with ``validation_auc`` (new) also
  ``validation auc at step %d: %.8f`` and an early stop at ``auc_tolerance``; with ``validation_gauc`` (new,
  needs ``validation_group_files``) then ``validation gauc at step %d: %.8f`` -- the grouped AUC of the same
  forward's scores -- and an early stop at ``gauc_tolerance``; with ``validation_ap`` (new) then ``validation ap
  at step %d: %.8f`` -- the average precision of the same scores -- and an early stop at ``ap_tolerance``;
* automatic restore of the latest checkpoint in ``log_dir`` (MonitoredTrainingSession);
* end: ``Average speed:  <ex/s>  ex/s`` and ``Model saved to  <log_dir>``;
* ``-t FILE``: chrome-trace timeline (reference: first step only; here the
  first few steps after one warm-up step);
* predict: ``<predict_file>_score`` with one raw score (logit) per line;
* evaluate (new): loss, ROC AUC and -- with ``predict_group_files`` -- grouped AUC of a checkpoint on the
  labelled predict files, and ``<predict_file>_gauc`` with one line per group; with ``threshold_metrics`` or
  targets also average precision, KS, best F1, the targets' operating points and ``<predict_file>_thresholds``;
  with ``auc_interval`` DeLong's standard error and confidence interval of the AUC, with ``baseline_score_files``
  DeLong's paired test against another model's scores;
* calibrate (new): an exact isotonic fit of the checkpoint's scores on the validation files, written as
  ``calibration.json`` into the checkpoint's directory; ``predict --calibrated`` then also writes
  ``<predict_file>_prob`` with one calibrated probability per line.

Multi-rank runs are synchronous: every step all ranks agree (one tiny
all-reduce) that each still has a batch, so the run ends cleanly when the first
rank's data is exhausted (the reference's OutOfRangeError, run_tffm.py:43-44).
"""

from __future__ import annotations

import os
import time

import numpy as np
import torch
import torch.distributed as dist

from .config import FMRunConfig
from .utils.fault import maybe_inject
from .utils.trace import roctx_range
from .data.reader import NativeTextReader, Prefetcher, ReaderState, TextBatchReader, load_file_batch
from .models.fm import FactorizationMachine
from .data.groups import load_group_files
from .calibration import FILE_NAME as CALIBRATION_FILE, CalibrationError, Calibrator, log_loss_sum_of_blocks
from .ops.kernels import auc, auc_delong, check_device_errors, gauc, isotonic_fit, rank_metrics, threshold_metrics
from .parallel.dist import DistContext, gather_dealt
from .utils import checkpoint as ckpt
from .utils.metrics import MetricsLogger


def _resolve_device(cfg: FMRunConfig, ctx: DistContext | None) -> torch.device:
    if ctx is not None and ctx.world > 1:
        return ctx.device
    if cfg.device in ("cpu", "cuda"):
        return torch.device("cuda" if cfg.device == "cuda" else "cpu")
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


# Version of the loader's shuffle draws (csrc/cpu/loader.cpp ``bounded``): 1 = ``rng() % range``
# (round 2), 2 = multiply-high.  Stored with every reader position; a resume across versions warns.
DRAW_VERSION = 2


class Trainer:
    def __init__(self, cfg: FMRunConfig, ctx: DistContext | None = None, *, monitor: bool = False,
                 trace: str | None = None, printer=print, trace_steps: int = 5):
        self.cfg = cfg
        self.ctx = ctx
        self.world = ctx.world if ctx is not None else 1
        self.rank = ctx.rank if ctx is not None else 0
        self.monitor = monitor
        self.trace = trace
        self.trace_steps = trace_steps
        self.print = printer if self.rank == 0 else (lambda *a, **k: None)
        self.device = _resolve_device(cfg, ctx)
        self.model = FactorizationMachine(cfg.fm_config(), device=self.device,
                                          dist=ctx if self.world > 1 else None)
        self.reader_state = ReaderState()
        self.restored_from = None
        self.val_groups = None  # (this rank's validation group ids, number of groups): load_validation

    def close(self) -> None:
        """Release the model's executor resources (graphs, exchange, streams)."""
        self.model.close()

    def __enter__(self) -> "Trainer":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # ------------------------------------------------------------------
    def restore(self) -> bool:
        path = ckpt.latest_checkpoint(self.cfg.log_dir)
        if path is None:
            return False
        meta = ckpt.restore_checkpoint(self.model, path)
        # this rank's own reader position (each rank reads its own file subset); a checkpoint
        # from another world size (or without per-rank entries) falls back to rank 0's
        per_rank = meta.get("reader_states") or {}
        if int(meta.get("reader_world", 1)) == self.world and str(self.rank) in per_rank:
            rs = per_rank[str(self.rank)] or {}
        else:
            rs = meta.get("reader_state") or {}
            if self.world > 1:
                self.print(f"Checkpoint reader positions are for world {meta.get('reader_world', 1)}; "
                           f"every rank resumes at rank 0's position")
        self.reader_state = ReaderState(epoch=int(rs.get("epoch", 0)),
                                        batches_in_epoch=int(rs.get("batches_in_epoch", 0)))
        dv = rs.get("draw_version") if rs else None
        if rs and dv is None:
            # (checkpoints written before the field existed: the draws may or may not be this build's)
            self.print(f"Note: checkpoint reader position does not record its shuffle draw version; resuming "
                       f"with this build's draws (version {DRAW_VERSION})")
        elif rs and int(dv) != DRAW_VERSION:
            # the loader's shuffle draws changed between the builds: the same seed gives another line
            # order, so replaying batches_in_epoch batches does not land on the same examples
            self.print(f"Warning: checkpoint reader position was written with shuffle draw version "
                       f"{dv} (this build: {DRAW_VERSION}); the resumed epoch repeats or skips some examples")
        self.restored_from = path
        self.print(f"Restored checkpoint {path} (global step {self.model.global_step})")
        return True

    def save(self) -> str | None:
        if not self.cfg.log_dir:
            return None
        rs = {"epoch": self.reader_state.epoch, "batches_in_epoch": self.reader_state.batches_in_epoch,
              "draw_version": DRAW_VERSION}
        return ckpt.save_checkpoint(self.model, self.cfg.log_dir, self.model.global_step, reader_state=rs,
                                    ctx=self.ctx if self.world > 1 else None,
                                    table_format=getattr(self.cfg, "checkpoint_format", "dense"))

    def _all_have_batch(self, have: bool) -> bool:
        if self.world == 1:
            return have
        t = torch.tensor([1 if have else 0], dtype=torch.int32, device=self.ctx.device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=self.ctx.group)
        return bool(t.item())

    def _global_loss(self, loss_sum: float, n: int) -> float:
        if self.world == 1:
            return loss_sum / max(n, 1)
        t = torch.tensor([loss_sum, float(n)], dtype=torch.float64, device=self.ctx.device)
        dist.all_reduce(t, group=self.ctx.group)
        return float(t[0] / max(t[1], 1.0))

    # ------------------------------------------------------------------
    def load_validation(self):
        c = self.cfg
        if not c.validation_data_files:
            return None
        self.print("Preloading validation data...")
        b = load_file_batch(c.validation_data_files, c.validation_weight_files, c.vocabulary_size,
                            c.hash_feature_id, c.parse_threads)
        ids = None
        if c.validation_group_files:
            # (densified over the whole set before the deal: every rank sees the same ids)
            gi = load_group_files(c.validation_group_files, c.validation_data_files)
            if gi.ids.size != b.B:
                raise ValueError("validation group files have %d lines, validation files %d examples"
                                 % (gi.ids.size, b.B))
            ids, num_groups = torch.from_numpy(gi.ids), gi.num_groups
        if self.world > 1:
            idx = torch.arange(self.rank, b.B, self.world)
            b = _take(b, idx)
            ids = None if ids is None else ids[idx].contiguous()
        self.val_groups = None if ids is None else (ids.to(self.device), num_groups)
        return b.to(self.device)

    def _device_cache(self):
        """The device to keep .fmb training files on, or None ([Train] device_cache)."""
        c = self.cfg
        if c.device_cache == "false" or self.device.type != "cuda" or not c.train_files:
            return None
        from .data import bincache, device_cache

        if not all(bincache.is_bin_file(f) for f in c.train_files):
            return None
        if c.device_cache == "auto":
            free, _ = torch.cuda.mem_get_info(self.device)
            if device_cache.dataset_bytes(c.train_files) > 0.4 * free:
                return None
        return self.device

    def validation_loss(self, vb) -> float:
        fo = self.model.forward(vb, loss=self.cfg.loss_type)
        return self._global_loss(float(fo.loss_sum), vb.B)

    def validation_metrics(self, vb) -> tuple[float, float]:
        """(validation loss, validation ROC AUC) from ONE forward: the loss as ``validation_loss`` gives
        it, the AUC (ops/kernels.py ``auc``, exact and weighted like the loss) over the forward's scores.
        Multi-rank: an exact AUC is no sum of per-rank AUCs, so every rank gathers all ranks' scores,
        labels and weights and computes the same AUC on the full set."""
        loss, v_auc, _ = self.validation_report(vb)
        return loss, v_auc

    def validation_report(self, vb, want_auc: bool = True, groups=None, *, rank_cutoffs=None,
                          want_gauc: bool = True, thresholds=None, delong=None) -> tuple:
        """(loss, ROC AUC or None, ``GaucStats`` or None) of a labelled batch from ONE forward.  ``groups``:
        ``(this rank's int32 group ids of vb's examples, number of groups)`` for the grouped AUC
        (ops/kernels.py ``gauc``) of the same scores.  Multi-rank: the ids travel with the scores, labels
        and weights (as their bit patterns: ``gather_dealt`` moves fp32 vectors and does no arithmetic).
        With ``rank_cutoffs`` (needs ``groups``) the tuple gains a fourth entry, the ``RankStats`` of
        ``rank_metrics`` on the same gathered scores (no example weights enter it); ``want_gauc`` False leaves
        the third entry None.  With ``thresholds`` = ``(precision targets, recall targets)`` the tuple gains
        a last entry, the ``ThresholdStats`` of ``threshold_metrics`` on the same gathered scores, labels and
        weights.  With ``delong`` = ``(every example's baseline score in file order, or None,)`` one more entry
        follows, the ``DelongStats`` of ``auc_delong`` on the same gathered scores and labels (unweighted: the
        caller's weights are all ones)."""
        fo = self.model.forward(vb, loss=self.cfg.loss_type)
        loss = self._global_loss(float(fo.loss_sum), vb.B)

        def thr(scores, labels, weights) -> tuple:
            if thresholds is None:
                return ()
            return (threshold_metrics(scores, labels, weights, precision_targets=thresholds[0],
                                      recall_targets=thresholds[1]),)

        def dlg(scores, labels) -> tuple:
            return () if delong is None else (auc_delong(scores, labels, delong[0]),)

        if rank_cutoffs is not None:
            if groups is None:
                raise ValueError("rank_cutoffs needs the group ids")
            scores, labels, weights, ids = gather_dealt(
                self.ctx if self.world > 1 else None,
                [fo.pred[:vb.B].contiguous(), vb.labels, vb.weights, groups[0].view(torch.float32)])
            ids = ids.view(torch.int32)
            return (loss, auc(scores, labels, weights).value() if want_auc else None,
                    gauc(scores, labels, ids, groups[1], weights) if want_gauc else None,
                    rank_metrics(scores, labels, ids, groups[1], rank_cutoffs)) + thr(scores, labels, weights) \
                + dlg(scores, labels)
        if not want_auc and groups is None and thresholds is None and delong is None:
            return loss, None, None
        ids = None if groups is None else groups[0].view(torch.float32)
        scores, labels, weights, ids = gather_dealt(self.ctx if self.world > 1 else None,
                                                    [fo.pred[:vb.B].contiguous(), vb.labels, vb.weights, ids])
        v_auc = auc(scores, labels, weights).value() if want_auc else None
        st = None if groups is None else gauc(scores, labels, ids.view(torch.int32), groups[1], weights)
        return (loss, v_auc, st) + thr(scores, labels, weights) + dlg(scores, labels)

    # ------------------------------------------------------------------
    def train(self) -> dict:
        c = self.cfg
        self.restore()
        vb = self.load_validation()
        kw = dict(vocab_size=c.vocabulary_size, hash_feature_id=c.hash_feature_id, num_epochs=c.num_epochs,
                  shuffle=c.shuffle, seed=c.seed, parse_threads=c.parse_threads, rank=self.rank, world=self.world,
                  state=ReaderState(self.reader_state.epoch, self.reader_state.batches_in_epoch))
        if c.loader == "native":
            reader = NativeTextReader(c.train_files, c.weight_files or None, c.batch_size,
                                      gpu_parse=self.device if c.gpu_parse else None,
                                      feed_device=self.device if self.device.type == "cuda" else None,
                                      device_cache=self._device_cache(), **kw)
            if reader.dds is not None:
                self.print(f"Training data resident on {self.device}: {reader.dds.N} examples, "
                           f"{reader.dds.nbytes / 2**30:.2f} GiB")
        else:
            reader = TextBatchReader(c.train_files, c.weight_files or None, c.batch_size, **kw)
        pf = Prefetcher(reader, self.device, queue_size=max(1, min(c.queue_size, 64)))
        metrics = MetricsLogger(c.log_dir if self.rank == 0 else None, every=c.save_summaries_steps)
        self.print("========", "train", "========")
        st = time.time()
        start_step = self.model.global_step
        step_num = start_step
        it = iter(pf)
        prof = None
        ended_early = False
        last_loss = float("nan")

        def fetch():
            with roctx_range("input_wait"):
                try:
                    nb = next(it)
                except StopIteration:
                    nb = None
            return nb, self._all_have_batch(nb is not None)

        def report(p):
            """Print / log a finished step.  Called once the NEXT step is enqueued, so reading
            this step's loss (a host sync) overlaps the device work of the next one."""
            sn, o, t0 = p
            loss = o.mean_loss()  # the reference fetches the loss every step
            tend = time.time()
            if self.monitor:
                q = pf.size()
                self.print("speed:", c.batch_size * self.world / max(tend - t0, 1e-9),
                           "shuffle_queue: %.2f%%" % (100.0 * pf.shuffle_fill()),
                           "example_queue: %.2f%%" % (q * 100.0 / pf.queue_size))
            if c.log_steps <= 1 or sn % c.log_steps == 0:
                self.print("-- Global Step: %d; Avg loss: %.5f;" % (sn, loss))
            metrics.log(sn, loss=loss, exq_size=pf.size(), shuffle_fill=pf.shuffle_fill())
            return loss, tend

        batch, have = fetch()
        nxt, nhave = fetch() if have else (None, False)
        pending = None
        tprev = time.time()
        # steady state: from the end of the first epoch (input caches, page cache, lazy
        # kernel loads and allocator growth are warm by then) to the end of the run
        steady_t0, steady_step = None, None
        while have:
            # lookahead: the next two batches (when every rank has them) let the executors build
            # their dedup / id exchange / early row exchange while this step computes
            nxt2, nhave2 = fetch() if nhave else (None, False)
            if self.trace and prof is None and step_num == start_step + 1:
                prof = _start_profiler()
            with roctx_range("train_step"):
                out = self.model.train_step(batch, nxt if nhave else None, nxt2 if nhave2 else None)
            step_num = self.model.global_step
            if batch.reader_pos is not None:  # position of the last CONSUMED batch (the reader runs ahead)
                self.reader_state.epoch, self.reader_state.batches_in_epoch = batch.reader_pos
                if steady_t0 is None and batch.reader_pos[0] >= 1:
                    if self.device.type == "cuda":
                        torch.cuda.synchronize(self.device)
                    steady_t0, steady_step = time.time(), step_num - 1
            if pending is not None:
                last_loss, tprev = report(pending)
            pending = (step_num, out, tprev)
            if prof is not None and step_num >= start_step + 1 + self.trace_steps:
                _stop_profiler(prof, self.trace)
                prof = None
                self.trace = None
            if step_num % max(c.save_steps, 1) == 0:
                last_loss, tprev = report(pending)
                pending = None
                if vb is not None:
                    v_gauc = v_ndcg = v_ap = None
                    want_thr = ((), ()) if c.validation_ap else None  # (no targets: the average precision)
                    if c.validation_ndcg is not None:
                        v_loss, v_auc, gstats, rstats, *tstats = self.validation_report(
                            vb, c.validation_auc, self.val_groups, rank_cutoffs=(c.validation_ndcg,),
                            want_gauc=c.validation_gauc, thresholds=want_thr)
                        v_gauc = gstats.value() if c.validation_gauc else None
                        v_ndcg = rstats.ndcg(c.validation_ndcg)
                    elif c.validation_gauc:
                        v_loss, v_auc, gstats, *tstats = self.validation_report(vb, c.validation_auc, self.val_groups,
                                                                                thresholds=want_thr)
                        v_gauc = gstats.value()
                    elif c.validation_ap:
                        v_loss, v_auc, _, *tstats = self.validation_report(vb, c.validation_auc, thresholds=want_thr)
                    elif c.validation_auc:
                        v_loss, v_auc = self.validation_metrics(vb)
                    else:
                        v_loss, v_auc = self.validation_loss(vb), None
                    if c.validation_ap:
                        v_ap = tstats[0].ap()
                    self.print("validation loss at step %d: %.8f" % (step_num, v_loss))
                    metrics.log(step_num, force=True, validation_loss=v_loss)
                    if v_auc is not None:
                        self.print("validation auc at step %d: %.8f" % (step_num, v_auc))
                        metrics.log(step_num, force=True, validation_auc=v_auc)
                    if v_gauc is not None:
                        self.print("validation gauc at step %d: %.8f" % (step_num, v_gauc))
                        metrics.log(step_num, force=True, validation_gauc=v_gauc)
                    if v_ndcg is not None:
                        self.print("validation ndcg@%d at step %d: %.8f" % (c.validation_ndcg, step_num, v_ndcg))
                        metrics.log(step_num, force=True, validation_ndcg=v_ndcg)
                    if v_ap is not None:
                        self.print("validation ap at step %d: %.8f" % (step_num, v_ap))
                        metrics.log(step_num, force=True, validation_ap=v_ap)
                    if c.tolerance is not None and v_loss < c.tolerance:
                        self.print("Loss on validation data set is below tolerance. Training completed.")
                        ended_early = True
                    if c.auc_tolerance is not None and v_auc is not None and v_auc >= c.auc_tolerance:
                        self.print("AUC on validation data set is above tolerance. Training completed.")
                        ended_early = True
                    if c.gauc_tolerance is not None and v_gauc is not None and v_gauc >= c.gauc_tolerance:
                        self.print("GAUC on validation data set is above tolerance. Training completed.")
                        ended_early = True
                    if c.ndcg_tolerance is not None and v_ndcg is not None and v_ndcg >= c.ndcg_tolerance:
                        self.print("NDCG on validation data set is above tolerance. Training completed.")
                        ended_early = True
                    if c.ap_tolerance is not None and v_ap is not None and v_ap >= c.ap_tolerance:
                        self.print("Average precision on validation data set is above tolerance. Training "
                                   "completed.")
                        ended_early = True
                check_device_errors(self.device)  # (kernels' sticky error word: fail before saving)
                if c.log_dir:
                    self.save()
            maybe_inject(step_num, self.rank)
            if ended_early or (c.max_steps is not None and step_num - start_step >= c.max_steps):
                break
            batch, have = nxt, nhave
            nxt, nhave = nxt2, nhave2
        if pending is not None:
            last_loss, _ = report(pending)
        if prof is not None:
            _stop_profiler(prof, self.trace)
        pf.close()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        check_device_errors(self.device)
        total = time.time() - st
        speed = (step_num - start_step) * c.batch_size * self.world / max(total, 1e-9)
        self.print("Average speed: ", speed, " ex/s")
        steady = None
        if steady_t0 is not None and step_num - steady_step > 0:
            steady = (step_num - steady_step) * c.batch_size * self.world / max(time.time() - steady_t0, 1e-9)
            self.print("Steady-state speed (epochs 2+): ", steady, " ex/s")
        if c.log_dir:
            self.save()
        self.print("Model saved to ", c.log_dir)
        metrics.close()
        return {"steps": step_num - start_step, "global_step": step_num, "avg_speed": speed, "steady_speed": steady,
                "last_loss": last_loss, "early_stop": ended_early}

    # ------------------------------------------------------------------
    def predict(self, calibrated: bool = False) -> list[str]:
        """``run.py predict``: ``<file>_score`` with one raw score per line.  ``calibrated``: also
        ``<file>_prob`` with the calibrated probability of every score, from the ``calibration.json`` that
        ``calibrate`` wrote into the restored checkpoint's directory."""
        c = self.cfg
        if not self.restore():
            raise FileNotFoundError(f"no checkpoint found in {c.log_dir}")
        cal = None
        if calibrated:
            cal_path = os.path.join(self.restored_from, CALIBRATION_FILE)
            if not os.path.exists(cal_path):
                raise CalibrationError(f"predict --calibrated: no {CALIBRATION_FILE} in {self.restored_from}; run "
                                       "'calibrate' on this checkpoint first")
            cal = Calibrator.load(cal_path)
        self.print("========", "predict", "========")
        written = []
        for path in c.predict_files:
            b = load_file_batch([path], None, c.vocabulary_size, c.hash_feature_id, c.parse_threads)
            if self.world > 1:
                idx = torch.arange(self.rank, b.B, self.world)
                mine = _take(b, idx).to(self.device)
                scores = self.model.predict(mine).cpu().numpy()
                parts = [None] * self.world
                dist.all_gather_object(parts, scores, group=self.ctx.cpu_group)
                full = np.empty(b.B, dtype=np.float32)
                for r, p in enumerate(parts):
                    full[r::self.world] = p
                scores = full
            else:
                scores = self.model.predict(b.to(self.device)).cpu().numpy()
            if self.rank == 0:
                out = path + "_score"
                with open(out, "w") as f:
                    for s in scores:
                        f.write(str(np.float32(s)) + "\n")
                written.append(out)
                if cal is not None:
                    probs = cal(torch.from_numpy(np.ascontiguousarray(scores, np.float32)).to(self.device))
                    with open(path + "_prob", "w") as f:
                        for p in probs.cpu().numpy():
                            f.write(str(np.float32(p)) + "\n")
                    written.append(path + "_prob")
        self.print("Done. Scores saved to same directory as predict files")
        return written

    # ------------------------------------------------------------------
    def calibrate(self) -> dict:
        """``run.py calibrate``: fit the monotone map from the restored model's raw score to P(positive) on the
        validation files (+ ``validation_weight_files``) -- an exact isotonic regression of ONE forward's scores
        (ops/kernels.py ``isotonic_fit``) -- and write it as ``calibration.json`` into the checkpoint's directory
        (it belongs to that step and is pruned with it) and, one line per block ``score_lo score_hi probability
        weight positives``, as ``<log_dir>/calibration_blocks.txt`` (the reliability table).  Prints
        ``calibrate: examples N blocks M loss L_before -> L_after ratio R_before -> 1.00000000 (in-sample)``:
        the validation loss of that forward, the same loss of the fitted values (from the blocks; a block whose
        value is 0 or 1 adds 0), and the predicted over the observed positive weight before the fit (after it,
        it is 1 by construction).  Multi-rank runs deal the examples as the validation does; rank 0 writes."""
        c = self.cfg
        if c.loss_type != "logistic":
            raise CalibrationError(f"calibrate: needs loss_type = logistic (raw scores that are logits of a "
                                   f"probability); this config has loss_type = {c.loss_type}")
        if not c.validation_data_files:
            raise CalibrationError("calibrate: needs [Train] validation_files, the held-out labelled set to fit on")
        if not self.restore():
            raise FileNotFoundError(f"no checkpoint found in {c.log_dir}")
        vb = self.load_validation()
        self.print("========", "calibrate", "========")
        fo = self.model.forward(vb, loss=c.loss_type)
        loss = self._global_loss(float(fo.loss_sum), vb.B)
        scores, labels, weights = gather_dealt(self.ctx if self.world > 1 else None,
                                               [fo.pred[:vb.B].contiguous(), vb.labels, vb.weights])
        fit = isotonic_fit(scores, labels, weights)
        try:
            blocks = fit.count()
        except ValueError as e:  # (a NaN score: there is no fit)
            raise CalibrationError(f"calibrate: {e}") from None
        if blocks == 0:
            raise CalibrationError("calibrate: the validation examples carry no weight")
        lo, hi, bw, by, bv = (t.cpu().numpy() for t in fit.blocks())
        total_w, pos_w = fit.totals()
        n = scores.numel()
        sig = torch.sigmoid(scores.to(torch.float64))
        predicted = float((sig if weights is None else sig * weights.to(torch.float64)).sum())
        ratio = predicted / pos_w if pos_w > 0 else float("nan")
        # (the validation loss is the weighted loss sum over the number of examples: the same mean here)
        after = log_loss_sum_of_blocks(bw, by, bv) / n
        cal = Calibrator.from_fit(fit, examples=n, global_step=int(self.model.global_step),
                                  loss_before=loss, loss_after=after, ratio_before=ratio)
        res = {"examples": n, "blocks": blocks, "loss_before": loss, "loss_after": after, "ratio_before": ratio,
               "calibrator": cal}
        if self.rank == 0:
            res["file"] = cal.save(os.path.join(self.restored_from, CALIBRATION_FILE))
            res["blocks_file"] = os.path.join(c.log_dir, "calibration_blocks.txt")
            with open(res["blocks_file"], "w") as f:
                for b in range(blocks):
                    f.write("%s %s %s %s %s\n" % (str(np.float32(lo[b])), str(np.float32(hi[b])),
                                                  str(np.float32(bv[b])), bw[b], by[b]))
        self.print("calibrate: examples %d blocks %d loss %.8f -> %.8f ratio %.8f -> 1.00000000 (in-sample)"
                   % (n, blocks, loss, after, ratio))
        return res

    # ------------------------------------------------------------------
    def evaluate(self) -> dict:
        """``run.py evaluate``: loss and ROC AUC of the restored model on every (labelled) predict file, from
        one forward with unit weights, printed as ``evaluate <file>: examples N loss L auc A``.  With ``[Predict]
        predict_group_files`` the line goes on `` gauc G valid_groups V/T coverage C`` and ``<file>_gauc`` gets
        one line per group, ``key auc positives negatives examples``, by ascending AUC then key; the groups
        without a positive or without a negative follow, by key, with ``nan``.  With ``[Predict] rank_cutoffs``
        the line then goes on `` ndcg@K v recall@K v precision@K v`` per cutoff and `` ranked_groups V/T`` (the
        means over the groups with a positive, ops/kernels.py ``rank_metrics``), and ``<file>_rank`` gets one
        line per group, ``key examples positives`` then ``ndcg@K recall@K precision@K`` per cutoff, by
        ascending NDCG at the first cutoff then key; the groups without a positive follow, by key, with
        ``nan``.  With ``[Predict] threshold_metrics`` (or targets) the line ends with `` ap A ks K best_f1 F``,
        then `` recall@p<pi> R`` per precision target and `` precision@r<rho> Q`` per recall target
        (ops/kernels.py ``threshold_metrics``), and ``<file>_thresholds`` gets one line per operating point.
        With ``[Predict] auc_interval = L`` the line then goes on `` auc_se S auc_lo A auc_hi B``: DeLong's
        standard error of the AUC and the interval at level L (ops/kernels.py ``auc_delong``); with ``[Predict]
        baseline_score_files`` (one raw score per line, as ``predict`` writes them) it ends with `` baseline_auc A
        auc_diff D diff_se S z Z p P``: the baseline's AUC on the same examples, this model's AUC minus it, and
        DeLong's paired test of the difference.
        Returns the metrics per file.
        Multi-rank runs deal the examples as ``predict`` does; rank 0 writes."""
        c = self.cfg
        if not self.restore():
            raise FileNotFoundError(f"no checkpoint found in {c.log_dir}")
        self.print("========", "evaluate", "========")
        results = {}
        for k, path in enumerate(c.predict_files):
            b = load_file_batch([path], None, c.vocabulary_size, c.hash_feature_id, c.parse_threads)
            gi = ids = None
            if c.predict_group_files:
                gi = load_group_files([c.predict_group_files[k]], [path])
                if gi.ids.size != b.B:
                    raise ValueError(f"{c.predict_group_files[k]}: {gi.ids.size} lines but {path} has {b.B} examples")
                ids = torch.from_numpy(gi.ids)
            mine = b
            if self.world > 1:
                idx = torch.arange(self.rank, b.B, self.world)
                mine = _take(b, idx)
                ids = None if ids is None else ids[idx].contiguous()
            groups = None if ids is None else (ids.to(self.device), gi.num_groups)
            rst = None
            want_thr = (tuple(c.precision_targets), tuple(c.recall_targets)) if c.threshold_metrics else None
            want_dl = None
            if c.auc_interval is not None or c.baseline_score_files:
                base = None
                if c.baseline_score_files:  # (every rank reads the whole file: the scores are gathered on each)
                    base = _read_scores(c.baseline_score_files[k])
                    if base.size != b.B:
                        raise ValueError(f"{c.baseline_score_files[k]}: {base.size} lines but {path} has {b.B} "
                                         "examples")
                    base = torch.from_numpy(base).to(self.device)
                want_dl = (base,)
            if c.rank_cutoffs:
                loss, v_auc, st, rst, *tst = self.validation_report(mine.to(self.device), True, groups,
                                                                    rank_cutoffs=tuple(c.rank_cutoffs),
                                                                    thresholds=want_thr, delong=want_dl)
            else:
                loss, v_auc, st, *tst = self.validation_report(mine.to(self.device), True, groups,
                                                               thresholds=want_thr, delong=want_dl)
            dst = tst.pop() if want_dl is not None else None
            res = {"examples": b.B, "loss": loss, "auc": v_auc}
            line = "evaluate %s: examples %d loss %.8f auc %.8f" % (path, b.B, loss, v_auc)
            if st is not None:
                res.update(gauc=st.value(), valid_groups=st.valid_groups(), groups=gi.num_groups,
                           coverage=st.coverage())
                line += " gauc %.8f valid_groups %d/%d coverage %.8f" % (res["gauc"], res["valid_groups"],
                                                                        gi.num_groups, res["coverage"])
                if self.rank == 0:
                    res["gauc_file"] = _write_group_aucs(path + "_gauc", gi, st.per_group().cpu().tolist())
            if rst is not None:
                for kk in rst.cutoffs:
                    res.update({"ndcg@%d" % kk: rst.ndcg(kk), "recall@%d" % kk: rst.recall(kk),
                                "precision@%d" % kk: rst.precision(kk)})
                    line += " ndcg@%d %.8f recall@%d %.8f precision@%d %.8f" % (
                        kk, res["ndcg@%d" % kk], kk, res["recall@%d" % kk], kk, res["precision@%d" % kk])
                res["ranked_groups"] = rst.ranked_groups()
                line += " ranked_groups %d/%d" % (res["ranked_groups"], gi.num_groups)
                if self.rank == 0:
                    res["rank_file"] = _write_group_ranks(path + "_rank", gi, rst.cutoffs,
                                                          rst.per_group().cpu().tolist())
            if tst:
                ts = tst[0]
                res.update(ap=ts.ap(), ks=ts.ks()[0], best_f1=ts.best_f1()[0])
                line += " ap %.8f ks %.8f best_f1 %.8f" % (res["ap"], res["ks"], res["best_f1"])
                for t in ts.precision_targets:
                    res["recall@p%g" % t] = ts.at_precision(t)[2]
                    line += " recall@p%g %.8f" % (t, res["recall@p%g" % t])
                for t in ts.recall_targets:
                    res["precision@r%g" % t] = ts.at_recall(t)[1]
                    line += " precision@r%g %.8f" % (t, res["precision@r%g" % t])
                if self.rank == 0:
                    res["thresholds_file"] = _write_thresholds(path + "_thresholds", ts)
            if dst is not None and c.auc_interval is not None:
                lo, hi = dst.interval(c.auc_interval)
                res.update(auc_se=dst.std_error(), auc_lo=lo, auc_hi=hi)
                line += " auc_se %.8f auc_lo %.8f auc_hi %.8f" % (res["auc_se"], lo, hi)
            if dst is not None and c.baseline_score_files:
                diff, se, z, p = dst.difference()
                res.update(baseline_auc=dst.auc_other(), auc_diff=diff, diff_se=se, z=z, p=p)
                line += " baseline_auc %.8f auc_diff %.8f diff_se %.8f z %.4f p %.6g" % (res["baseline_auc"], diff,
                                                                                         se, z, p)
            self.print(line)
            results[path] = res
        return results


    # ------------------------------------------------------------------
    def explain(self, top: int | None = None) -> list[str]:
        """``run.py explain``: for every predict file, ``<file>_contrib`` (one line per example: the score, then
        ``id:contribution`` tokens in input order -- with ``top``, the ``top`` largest |contribution| of the
        line, by descending |c| then position) and ``<file>_importance`` (one line per distinct id:
        ``id count mean_abs mean``, by descending sum |c| then ascending id).  Ids are table rows (after
        hashing / modulo).  Multi-rank runs split the examples as ``predict`` does."""
        from .models.table import bits_for
        from .ops import kernels as K

        c = self.cfg
        if top is not None and top < 0:
            raise ValueError("explain: --top must be >= 0")
        if not self.restore():
            raise FileNotFoundError(f"no checkpoint found in {c.log_dir}")
        self.print("========", "explain", "========")
        written = []
        for path in c.predict_files:
            b = load_file_batch([path], None, c.vocabulary_size, c.hash_feature_id, c.parse_threads)
            idx = torch.arange(self.rank, b.B, self.world)
            mine = (_take(b, idx) if self.world > 1 else b).to(self.device)
            contrib, _ = self.model.explain(mine)
            pred = self.model.predict(mine)  # (the score ``predict`` writes, bit for bit)
            ids32 = mine.ids.to(torch.int32)
            if mine.nnz > 0:
                dd = K.dedup(ids32, key_bits=bits_for(max(c.vocabulary_size, 2)), want_perm=True)
                imp = [t.cpu().numpy() for t in K.feature_importance(contrib, dd)]
            else:
                imp = [np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0), np.empty(0)]
            part = (pred.cpu().numpy(), contrib.cpu().numpy(), imp)
            parts = [part]
            if self.world > 1:
                parts = [None] * self.world
                dist.all_gather_object(parts, part, group=self.ctx.cpu_group)
            if self.rank != 0:
                continue
            offs = b.offsets.numpy().astype(np.int64)
            ids = b.ids.numpy()
            scores = np.empty(b.B, dtype=np.float32)
            full = np.empty(b.nnz, dtype=np.float32)
            for r, (p_r, c_r, _) in enumerate(parts):
                scores[r::self.world] = p_r
                full[_occ_index(offs, np.arange(r, b.B, self.world))] = c_r
            out = path + "_contrib"
            with open(out, "w") as f:
                for i in range(b.B):
                    s, e = offs[i], offs[i + 1]
                    pos = np.arange(s, e)
                    if top is not None:
                        pos = pos[np.argsort(-np.abs(full[s:e]), kind="stable")[:top]]
                    toks = [f"{ids[j]}:{str(np.float32(full[j]))}" for j in pos]
                    f.write(" ".join([str(np.float32(scores[i]))] + toks) + "\n")
            written.append(out)
            # importance: the ranks' partial sums merged in rank order, fp64
            keys = np.concatenate([p[2][0].astype(np.int64) for p in parts])
            uniq, inv = np.unique(keys, return_inverse=True)
            count = np.zeros(uniq.size, dtype=np.int64)
            sum_abs = np.zeros(uniq.size, dtype=np.float64)
            total = np.zeros(uniq.size, dtype=np.float64)
            np.add.at(count, inv, np.concatenate([p[2][1].astype(np.int64) for p in parts]))
            np.add.at(sum_abs, inv, np.concatenate([p[2][2].astype(np.float64) for p in parts]))
            np.add.at(total, inv, np.concatenate([p[2][3].astype(np.float64) for p in parts]))
            out = path + "_importance"
            with open(out, "w") as f:
                for k in np.lexsort((uniq, -sum_abs)):
                    f.write(f"{uniq[k]} {count[k]} {str(np.float32(sum_abs[k] / count[k]))} "
                            f"{str(np.float32(total[k] / count[k]))}\n")
            written.append(out)
        self.print("Done. Contributions and importance saved to same directory as predict files")
        return written


    # ------------------------------------------------------------------
    def recommend(self, candidates: str, top: int = 10) -> list[str]:
        """``run.py recommend``: rank the candidates of file ``candidates`` (one per line, the predict files'
        format; the label column is read and ignored) for every line of the predict files.  Writes
        ``<file>_recommend``: line i holds up to ``top`` tokens ``c:score``, best first (equal scores by
        ascending c), c the 0-based line number of the candidate and the score that of the context's and the
        candidate's features taken together (``FactorizationMachine.recommend``).  Multi-rank runs deal the
        contexts as ``predict`` does; every rank profiles all candidates."""
        from .ops import kernels as K

        c = self.cfg
        if not isinstance(top, int) or not 1 <= top <= K.TOPK_MAX_K:
            raise ValueError(f"recommend: --top must be in 1..{K.TOPK_MAX_K}, got {top}")
        if not self.restore():
            raise FileNotFoundError(f"no checkpoint found in {c.log_dir}")
        self.print("========", "recommend", "========")
        cands = load_file_batch([candidates], None, c.vocabulary_size, c.hash_feature_id, c.parse_threads)
        preds, profs = [], []
        for s0 in range(0, cands.B, RECOMMEND_PROFILE_BATCH):  # (a collective per chunk on a row-sharded model)
            part = _take(cands, torch.arange(s0, min(s0 + RECOMMEND_PROFILE_BATCH, cands.B))).to(self.device)
            p, s = self.model.profile(part)
            preds.append(p)
            profs.append(s)
        if preds:
            index = (torch.cat(preds), torch.cat(profs))
        else:
            index = (torch.empty(0, dtype=torch.float32, device=self.device),
                     torch.empty((0, self.model.Kp), dtype=torch.float32, device=self.device))
        written = []
        for path in c.predict_files:
            b = load_file_batch([path], None, c.vocabulary_size, c.hash_feature_id, c.parse_threads)
            mine = (_take(b, torch.arange(self.rank, b.B, self.world)) if self.world > 1 else b).to(self.device)
            idx, score = self.model.recommend(mine, index, top)
            part = (idx.cpu().numpy(), score.cpu().numpy())
            parts = [part]
            if self.world > 1:
                parts = [None] * self.world
                dist.all_gather_object(parts, part, group=self.ctx.cpu_group)
            if self.rank != 0:
                continue
            full_i = np.empty((b.B, top), dtype=np.int32)
            full_s = np.empty((b.B, top), dtype=np.float32)
            for r, (i_r, s_r) in enumerate(parts):
                full_i[r::self.world] = i_r
                full_s[r::self.world] = s_r
            out = path + "_recommend"
            with open(out, "w") as f:
                for i in range(b.B):
                    f.write(" ".join(f"{ci}:{str(np.float32(sc))}" for ci, sc in zip(full_i[i], full_s[i]) if ci >= 0)
                            + "\n")
            written.append(out)
        self.print("Done. Recommendations saved to same directory as predict files")
        return written


def _write_group_aucs(out: str, gi, recs: list) -> str:
    """``<file>_gauc`` of ``Trainer.evaluate`` from the per-group ``[U2, P, N]`` records."""
    sizes = np.bincount(gi.ids, minlength=gi.num_groups)
    rows = []
    for g, (u2, p, n) in enumerate(recs):
        valid = p > 0 and n > 0
        rows.append((not valid, u2 / (2 * p * n) if valid else 0.0, gi.keys[g], g))
    with open(out, "w") as f:
        for invalid, a, key, g in sorted(rows):
            f.write("%s %s %s %s %d\n" % (key, "nan" if invalid else str(np.float32(a)), recs[g][1], recs[g][2],
                                          sizes[g]))
    return out


def _read_scores(path: str) -> np.ndarray:
    """The fp32 scores of a ``<file>_score`` file, one per line: what ``predict`` wrote, bit for bit (it prints
    the shortest decimal that reads back as the same fp32 value)."""
    with open(path) as f:
        return np.array([float(t) for t in f.read().split()], dtype=np.float64).astype(np.float32)


def _write_thresholds(out: str, ts) -> str:
    """``<file>_thresholds`` of ``Trainer.evaluate``: one line per operating point, ``kind target threshold
    precision recall f1 tp fp`` -- ``ks``, ``best_f1`` (target ``-``), a ``precision`` row per precision target
    and a ``recall`` row per recall target; floats as ``predict`` prints scores, ``nan`` where no threshold
    qualifies."""
    st = ts.stats()
    ok = ts._defined(st)
    rows = [("ks", "-", st["ks"]), ("best_f1", "-", st["best_f1"])]
    rows += [("precision", "%g" % t, p) for t, p in zip(ts.precision_targets, st["precision"])]
    rows += [("recall", "%g" % t, p) for t, p in zip(ts.recall_targets, st["recall"])]
    with open(out, "w") as f:
        for kind, target, point in rows:
            vals, counts = [float("nan")] * 4, ["nan", "nan"]
            if ok and point is not None:
                tp, fp, t = point
                vals = [t, tp / (tp + fp), tp / st["P"], 2 * tp / ((tp + fp) + st["P"])]
                counts = [str(int(v)) if float(v).is_integer() else repr(float(v)) for v in (tp, fp)]
            f.write("%s %s %s %s\n" % (kind, target, " ".join(str(np.float32(v)) for v in vals), " ".join(counts)))
    return out


def _write_group_ranks(out: str, gi, cutoffs: tuple, recs: list) -> str:
    """``<file>_rank`` of ``Trainer.evaluate`` from the per-group ``[n, P, (DCG, IDCG, hits) per cutoff]`` records
    (ordered by the NDCG as written, in fp32: the last bits of an fp64 ratio order nothing)."""
    rows = []
    for g, r in enumerate(recs):
        ranked = r[1] > 0
        vals = []
        for i, k in enumerate(cutoffs):
            dcg, idcg, hits = r[2 + 3 * i:5 + 3 * i]
            vals += [dcg / idcg, hits / r[1], hits / k] if ranked else [float("nan")] * 3
        rows.append((not ranked, float(np.float32(vals[0])) if ranked else 0.0, gi.keys[g], g, vals))
    with open(out, "w") as f:
        for unranked, _, key, g, vals in sorted(rows):
            f.write("%s %d %d %s\n" % (key, recs[g][0], recs[g][1],
                                       " ".join("nan" if unranked else str(np.float32(v)) for v in vals)))
    return out


RECOMMEND_PROFILE_BATCH = 65536  # candidate lines per forward pass of ``Trainer.recommend``


def _occ_index(offs: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """Occurrence positions of examples ``idx`` of a CSR batch, in ``_take``'s order."""
    sizes = offs[idx + 1] - offs[idx]
    ends = np.cumsum(sizes)
    total = int(ends[-1]) if idx.size else 0
    return np.repeat(offs[idx], sizes) + np.arange(total, dtype=np.int64) - np.repeat(ends - sizes, sizes)


def _take(b, idx: torch.Tensor):
    """Sub-batch of examples ``idx`` (host tensors)."""
    from .data.batch import Batch

    o = b.offsets.long()
    sizes = (o[1:] - o[:-1])[idx]
    starts = o[:-1][idx]
    # feature positions of the chosen examples, vectorised: start of each example repeated
    # over its features + the position inside the example
    ends = torch.cumsum(sizes, 0)
    total = int(ends[-1]) if idx.numel() else 0
    within = torch.arange(total, dtype=torch.long) - torch.repeat_interleave(ends - sizes, sizes)
    gather = torch.repeat_interleave(starts, sizes) + within
    offs = torch.zeros(idx.numel() + 1, dtype=torch.int32)
    offs[1:] = torch.cumsum(sizes, 0)
    return Batch(b.labels[idx], offs, b.ids[gather], None if b.vals is None else b.vals[gather],
                 None if b.weights is None else b.weights[idx], int(offs[-1]), max_feats=b.max_feats)


def _start_profiler():
    acts = [torch.profiler.ProfilerActivity.CPU]
    if torch.cuda.is_available():
        acts.append(torch.profiler.ProfilerActivity.CUDA)
    prof = torch.profiler.profile(activities=acts)
    prof.__enter__()
    return prof


def _stop_profiler(prof, trace: str) -> None:
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    prof.__exit__(None, None, None)
    if not trace.endswith(".json"):
        trace += ".json"
    d = os.path.dirname(trace)
    if d:
        os.makedirs(d, exist_ok=True)
    prof.export_chrome_trace(trace)
