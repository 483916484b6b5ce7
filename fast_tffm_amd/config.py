"""INI configuration, key-for-key compatible with the reference's sample.cfg.

Reference loader: ``Model._get_config`` (tffm/fm_model.py:367-475) with the
Python-2 ``ConfigParser``; every value read is echoed as ``  key = value`` under
a ``Config:`` header; comma lists are stripped, globbed and sorted.

Decisions on reference quirks:
* ``hash_feature_id`` is read by the reference but never passed to the parser
  (fm_model.py:400-401 vs :69-71); here it is wired through, as README.md:50
  promises.
* ``save_steps`` is "optional" but used unconditionally (int(None) crashes the
  reference): here it defaults to 100.
* weight/validation file count checks compare the *expanded* file lists, not
  the pattern counts (fm_model.py:447, :467).
* ``predict_files`` is truly optional (the reference crashes on None, :472-475).
* ``model_file`` is read and kept, unused, like the reference (:405-407).

Extensions (new keys, all optional):
  [General]     seed, device = auto|cpu|cuda,
                global_bias = true|false (learned b0; its gradient is all-reduced over ranks),
                dtype = fp32|bf16|fp8 (fp8: OCP e4m3 + per-row scale, GPU)
  [Train]       optimizer = adagrad|ftrl|sgd, ftrl.l1, ftrl.l2, ftrl.beta,
                ftrl.initial_accumulator, parse_threads, loader = native|python, gpu_parse = true|false,
                device_cache = auto|true|false, stochastic_rounding = true|false,
                shuffle = true|false,
                max_steps, dedup_chunk, log_steps,
                validation_auc = true|false (exact weighted ROC AUC of the validation scores, printed and logged
                                after the validation loss; default false), auc_tolerance = <float> (stop when
                                the validation AUC is >= it; needs validation_auc and validation_files),
                validation_group_files = <files> (one group key per line, parallel to validation_files),
                validation_gauc = true|false (grouped AUC of the validation scores, printed and logged after the
                                AUC / loss lines; needs validation_group_files; default false),
                gauc_tolerance = <float> (stop when the validation GAUC is >= it; needs validation_gauc),
                validation_ndcg = <K> (mean NDCG@K over the validation groups with a positive, printed and logged
                                after the GAUC / AUC / loss lines; one integer in [1, 4096]; needs
                                validation_group_files), ndcg_tolerance = <float> (stop when the validation
                                NDCG@K is >= it; needs validation_ndcg),
                validation_ap = true|false (average precision of the validation scores, weighted like the loss,
                                printed and logged after those lines; default false), ap_tolerance = <float>
                                (stop when it is >= this; needs validation_ap and validation_files),
                loss_type = mse|logistic|rank_softmax|rank_pairwise (rank_softmax: the listwise loss, a softmax
                                cross-entropy per group over the examples of one batch; rank_pairwise: the
                                logistic loss of every (positive, negative) pair of such a group, the smooth
                                surrogate of GAUC; both: local mode, one rank),
                rank_group_feature = <P> (the two rank losses only: an example's group key is the table row of its
                                P-th feature, 0-based; default 0; examples with fewer features are left out),
                checkpoint_format = dense|sparse (sparse: a checkpoint stores only the rows that differ from
                                their counter-based init, and restore regenerates the others; default dense)
  [Predict]     predict_group_files = <files> (one group key per line, parallel to predict_files: the
                                ``evaluate`` task then reports the grouped AUC and writes <file>_gauc),
                rank_cutoffs = <K>[,<K>...] (1 to 4 ascending integers in [1, 4096]: ``evaluate`` then also
                                reports NDCG@K, recall@K and precision@K per group and writes <file>_rank; needs
                                predict_group_files),
                threshold_metrics = true|false (``evaluate`` then also reports the average precision, KS and
                                the best F1 and writes <file>_thresholds; default false),
                precision_targets = <p>[,<p>...] / recall_targets = <r>[,<r>...] (0 to 4 values in (0, 1] each:
                                ``evaluate`` reports the recall at precision >= p / the precision at recall >= r
                                and the score thresholds in <file>_thresholds; either implies threshold_metrics),
                auc_interval = <L> (a confidence level in (0, 1): ``evaluate`` then also reports DeLong's standard
                                error of the AUC and the interval at that level),
                baseline_score_files = <files> (one raw score per line as ``predict`` writes them, parallel to
                                predict_files: ``evaluate`` then also reports the baseline's AUC and DeLong's
                                paired test of the difference)
  [Distributed] mode = auto|local|shard|dp|dp_dense, grad_reduce = sum|mean,
                comm_dtype = auto|fp32|bf16 (row-sharded wire rows; auto = table storage dtype),
                microbatches = 1|2|... (row-sharded step parts overlapping the exchange; default 1),
                prefetch_rows = auto|on|off (exchange the next step's rows early, re-send updated ones),
                overlap_grads = auto|on|off (split backward; first half's gradients sent while the rest runs;
                                auto = on with one microbatch),
                staleness = 0|1 (row-sharded step: 0 = synchronous; 1 = bounded staleness, the reference's
                                asynchronous updates made deterministic: step t reads every row with the
                                gradients of steps <= t-2 applied, step t-1's exchange + apply overlap it)
"""

from __future__ import annotations

import configparser
import glob
import os
from dataclasses import dataclass, field

GENERAL, TRAIN, PREDICT, DISTRIBUTED = "General", "Train", "Predict", "Distributed"


_TABLE_DTYPES = ("fp32", "bf16", "fp8")  # -> torch.float32 / bfloat16 / float8_e4m3fn
RANK_LOSSES = ("rank_softmax", "rank_pairwise")  # ops/kernels.py RANK_LOSSES: the group losses of one batch

class ConfigError(ValueError):
    pass


def _expand(patterns: list[str], base_dir: str | None = None) -> list[str]:
    out: list[str] = []
    for p in patterns:
        hits = glob.glob(p)
        if not hits and base_dir and not os.path.isabs(p):
            hits = glob.glob(os.path.join(base_dir, p))
        out.extend(hits)
    return sorted(out)


@dataclass
class FMRunConfig:
    # [General]
    vocabulary_size: int = 8000000
    vocabulary_block_num: int = 100
    factor_num: int = 10
    hash_feature_id: bool = False
    log_dir: str | None = None
    model_file: str | None = None
    save_summaries_steps: int = 100
    seed: int = 0
    dtype: str = "fp32"
    device: str = "auto"
    # [Train]
    batch_size: int = 50000
    init_value_range: float = 0.01
    factor_lambda: float = 0.0
    bias_lambda: float = 0.0
    num_epochs: int = 10
    learning_rate: float = 0.01
    adagrad_init_accumulator: float = 0.1
    loss_type: str = "mse"      # mse | logistic | rank_softmax (listwise) | rank_pairwise: per group of one batch
    rank_group_feature: int = 0  # rank losses: the feature position whose table row is the group key
    save_steps: int = 100
    queue_size: int = 10000
    shuffle_threads: int = 1
    train_files: list[str] = field(default_factory=list)
    weight_files: list[str] = field(default_factory=list)
    validation_data_files: list[str] = field(default_factory=list)
    validation_weight_files: list[str] = field(default_factory=list)
    tolerance: float | None = None
    optimizer: str = "adagrad"
    ftrl_l1: float = 0.0
    ftrl_l2: float = 0.0
    ftrl_beta: float = 0.0
    ftrl_initial_accumulator: float = 0.1
    parse_threads: int = 4
    loader: str = "native"      # native (C++ loader thread) | python
    gpu_parse: bool = False     # native loader: tokenize on the GPU (hip/parse.hip)
    device_cache: str = "auto"  # .fmb train files: keep them in HBM, gather batches on the device
                                # (auto: when they take <= 40% of the free device memory)
    stochastic_rounding: bool = True  # bf16 / fp8 tables: stochastically rounded updates
    shuffle: bool = True
    max_steps: int | None = None
    dedup_chunk: int = 32
    global_bias: bool = False
    log_steps: int = 1
    validation_auc: bool = False        # report the exact weighted ROC AUC next to the validation loss
    auc_tolerance: float | None = None  # stop when the validation AUC is >= this
    checkpoint_format: str = "dense"    # dense (every row) | sparse (rows that differ from their init)
    validation_group_files: list[str] = field(default_factory=list)  # one group key per validation line
    validation_gauc: bool = False        # report the grouped AUC of the validation scores
    gauc_tolerance: float | None = None  # stop when the validation GAUC is >= this
    validation_ndcg: int | None = None   # report the mean NDCG@K of the validation groups
    ndcg_tolerance: float | None = None  # stop when the validation NDCG@K is >= this
    # [Predict]
    predict_files: list[str] = field(default_factory=list)
    predict_group_files: list[str] = field(default_factory=list)  # one group key per predict line (evaluate)
    rank_cutoffs: list[int] = field(default_factory=list)  # NDCG@K / recall@K / precision@K cutoffs (evaluate)
    validation_ap: bool = False          # report the average precision of the validation scores
    ap_tolerance: float | None = None    # stop when the validation average precision is >= this
    threshold_metrics: bool = False      # evaluate: average precision, KS, best F1 and <file>_thresholds
    precision_targets: list[float] = field(default_factory=list)  # evaluate: recall at precision >= each
    recall_targets: list[float] = field(default_factory=list)     # evaluate: precision at recall >= each
    auc_interval: float | None = None    # evaluate: DeLong confidence interval of the AUC at this level
    baseline_score_files: list[str] = field(default_factory=list)  # evaluate: paired DeLong test against these scores
    # [Distributed]
    mode: str = "auto"
    grad_reduce: str = "sum"
    comm_dtype: str = "auto"
    microbatches: int = 0
    prefetch_rows: str = "auto"
    overlap_grads: str = "auto"
    staleness: int = 0
    config_file: str | None = None

    # ------------------------------------------------------------------
    def fm_config(self):
        """The model/step configuration (models.fm.FMConfig)."""
        import torch

        from .models.fm import FMConfig
        from .ops.kernels import OptConfig

        if self.optimizer == "ftrl":
            opt = OptConfig("ftrl", lr=self.learning_rate, l1=self.ftrl_l1, l2=self.ftrl_l2, beta=self.ftrl_beta,
                            initial_accumulator=self.ftrl_initial_accumulator)
        else:
            opt = OptConfig(self.optimizer, lr=self.learning_rate, initial_accumulator=self.adagrad_init_accumulator)
        return FMConfig(vocabulary_size=self.vocabulary_size, factor_num=self.factor_num, loss_type=self.loss_type,
                        rank_group_feature=self.rank_group_feature,
                        factor_lambda=self.factor_lambda, bias_lambda=self.bias_lambda, batch_size=self.batch_size,
                        init_value_range=self.init_value_range, seed=self.seed,
                        dtype={"fp32": torch.float32, "bf16": torch.bfloat16,
                               "fp8": torch.float8_e4m3fn}[self.dtype], opt=opt, mode=self.mode,
                        grad_reduce=self.grad_reduce, comm_dtype=self.comm_dtype, microbatches=self.microbatches,
                        prefetch_rows=self.prefetch_rows,
                        overlap_grads=self.overlap_grads, staleness=self.staleness,
                        stochastic_rounding=self.stochastic_rounding, dedup_chunk=self.dedup_chunk,
                        global_bias=self.global_bias)


def _cutoffs(option: str, items: list, most: int) -> list:
    """The ranking cutoffs of ``option``: 1 to ``most`` strictly ascending integers in [1, 4096]."""
    try:
        ks = [int(s) for s in items]
    except ValueError:
        ks = []
    if not 1 <= len(ks) <= most or any(not 1 <= k <= 4096 for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        what = "one integer" if most == 1 else "1 to %d strictly ascending integers" % most
        raise ConfigError("%s must be %s in [1, 4096], got %s." % (option, what, ",".join(items)))
    return ks


def _targets(option: str, items: list) -> list:
    """The precision / recall targets of ``option``: 1 to 4 numbers in (0, 1]."""
    try:
        ts = [float(s) for s in items]
    except ValueError:
        ts = []
    if not 1 <= len(ts) <= 4 or any(not 0.0 < t <= 1.0 for t in ts):
        raise ConfigError("%s must be 1 to 4 numbers in (0, 1], got %s." % (option, ",".join(items)))
    return ts


def load_config(config_file: str, *, echo: bool = True, printer=print) -> FMRunConfig:
    if not os.path.exists(config_file):
        raise ConfigError(f"config file not found: {config_file}")
    cp = configparser.ConfigParser(inline_comment_prefixes=(";",), strict=False)
    cp.read(config_file)
    base_dir = os.path.dirname(os.path.abspath(config_file))
    c = FMRunConfig(config_file=config_file)

    def read(section: str, option: str, required: bool = True):
        if not cp.has_option(section, option):
            if required:
                raise ConfigError("%s is undefined." % option)
            return None
        value = cp.get(section, option)
        if echo:
            printer("  {0} = {1}".format(option, value))
        return value

    def read_list(section: str, option: str, required: bool = True):
        v = read(section, option, required)
        if v is None:
            return None
        return [s.strip() for s in v.split(",") if s.strip()]

    def opt(section, option, conv, default):
        v = read(section, option, required=False)
        return default if v is None else conv(v)

    def to_bool(v: str) -> bool:
        return v.strip().lower() == "true"

    if echo:
        printer("Config: ")
    c.vocabulary_size = int(read(GENERAL, "vocabulary_size"))
    c.vocabulary_block_num = int(read(GENERAL, "vocabulary_block_num"))
    c.factor_num = int(read(GENERAL, "factor_num"))
    c.hash_feature_id = to_bool(read(GENERAL, "hash_feature_id"))
    c.log_dir = read(GENERAL, "log_dir", required=False)
    c.model_file = read(GENERAL, "model_file", required=False)
    c.save_summaries_steps = opt(GENERAL, "save_summaries_steps", int, c.save_summaries_steps)
    c.seed = opt(GENERAL, "seed", int, c.seed)
    c.global_bias = opt(GENERAL, "global_bias", to_bool, c.global_bias)
    c.dtype = opt(GENERAL, "dtype", lambda s: s.strip().lower(), c.dtype)
    c.device = opt(GENERAL, "device", lambda s: s.strip().lower(), c.device)

    c.batch_size = int(read(TRAIN, "batch_size"))
    c.init_value_range = float(read(TRAIN, "init_value_range"))
    c.factor_lambda = float(read(TRAIN, "factor_lambda"))
    c.bias_lambda = float(read(TRAIN, "bias_lambda"))
    c.num_epochs = int(read(TRAIN, "epoch_num"))
    c.learning_rate = float(read(TRAIN, "learning_rate"))
    c.adagrad_init_accumulator = float(read(TRAIN, "adagrad.initial_accumulator"))
    c.loss_type = read(TRAIN, "loss_type").strip().lower()
    c.save_steps = opt(TRAIN, "save_steps", int, c.save_steps)
    c.queue_size = opt(TRAIN, "queue_size", int, c.queue_size)
    c.shuffle_threads = opt(TRAIN, "shuffle_threads", int, c.shuffle_threads)
    c.optimizer = opt(TRAIN, "optimizer", lambda s: s.strip().lower(), c.optimizer)
    c.ftrl_l1 = opt(TRAIN, "ftrl.l1", float, c.ftrl_l1)
    c.ftrl_l2 = opt(TRAIN, "ftrl.l2", float, c.ftrl_l2)
    c.ftrl_beta = opt(TRAIN, "ftrl.beta", float, c.ftrl_beta)
    c.ftrl_initial_accumulator = opt(TRAIN, "ftrl.initial_accumulator", float, c.ftrl_initial_accumulator)
    c.parse_threads = opt(TRAIN, "parse_threads", int, c.parse_threads)
    c.loader = opt(TRAIN, "loader", lambda s: s.strip().lower(), c.loader)
    c.gpu_parse = opt(TRAIN, "gpu_parse", lambda s: s.strip().lower() == "true", c.gpu_parse)
    c.device_cache = opt(TRAIN, "device_cache", lambda s: s.strip().lower(), c.device_cache)
    if c.device_cache not in ("auto", "true", "false"):
        raise ConfigError(f"[Train] device_cache must be auto, true or false, got {c.device_cache}")
    c.stochastic_rounding = opt(TRAIN, "stochastic_rounding", lambda s: s.strip().lower() == "true",
                                c.stochastic_rounding)
    if c.loader not in ("native", "python"):
        raise ConfigError(f"[Train] loader must be native or python, got {c.loader}")
    c.shuffle = opt(TRAIN, "shuffle", to_bool, c.shuffle)
    c.max_steps = opt(TRAIN, "max_steps", int, c.max_steps)
    c.dedup_chunk = opt(TRAIN, "dedup_chunk", int, c.dedup_chunk)
    c.log_steps = opt(TRAIN, "log_steps", int, c.log_steps)
    c.validation_auc = opt(TRAIN, "validation_auc", to_bool, c.validation_auc)
    c.auc_tolerance = opt(TRAIN, "auc_tolerance", float, c.auc_tolerance)
    c.checkpoint_format = opt(TRAIN, "checkpoint_format", lambda s: s.strip().lower(), c.checkpoint_format)
    if c.checkpoint_format not in ("dense", "sparse"):
        raise ConfigError(f"[Train] checkpoint_format must be dense or sparse, got {c.checkpoint_format}")

    if c.loss_type not in ("logistic", "mse") + RANK_LOSSES:
        raise ConfigError("loss_type must be 'logistic', 'mse', 'rank_softmax' or 'rank_pairwise', got %r"
                          % c.loss_type)
    rgf = read(TRAIN, "rank_group_feature", required=False)
    if rgf is not None:
        if c.loss_type not in RANK_LOSSES:
            raise ConfigError("rank_group_feature needs loss_type = rank_softmax or rank_pairwise.")
        try:
            c.rank_group_feature = int(rgf)
        except ValueError:
            c.rank_group_feature = -1
        if c.rank_group_feature < 0:
            raise ConfigError("rank_group_feature must be an integer >= 0, got %s." % rgf.strip())
    if c.optimizer not in ("adagrad", "ftrl", "sgd"):
        raise ConfigError("optimizer must be adagrad|ftrl|sgd, got %r" % c.optimizer)
    if c.dtype not in _TABLE_DTYPES:
        raise ConfigError("dtype must be fp32|bf16|fp8, got %r" % c.dtype)

    c.train_files = _expand(read_list(TRAIN, "train_files"), base_dir)
    wf = read_list(TRAIN, "weight_files", required=False)
    if wf is not None:
        c.weight_files = _expand(wf, base_dir)
        if len(c.train_files) != len(c.weight_files):
            raise ConfigError("The numbers of train files and weight files do not match.")

    vf = read_list(TRAIN, "validation_files", required=False)
    if vf is not None:
        c.validation_data_files = _expand(vf, base_dir)
        c.tolerance = float(read(TRAIN, "tolerance"))
    vwf = read_list(TRAIN, "validation_weight_files", required=False)
    if vwf is not None:
        c.validation_weight_files = _expand(vwf, base_dir)
        if len(c.validation_data_files) != len(c.validation_weight_files):
            raise ConfigError("The numbers of validation data files and validation weight files do not match.")
    if c.auc_tolerance is not None and not (c.validation_auc and c.validation_data_files):
        raise ConfigError("auc_tolerance needs validation_auc = true and validation_files.")
    vgf = read_list(TRAIN, "validation_group_files", required=False)
    if vgf is not None:
        if not c.validation_data_files:
            raise ConfigError("validation_group_files needs validation_files.")
        c.validation_group_files = _expand(vgf, base_dir)
        if len(c.validation_data_files) != len(c.validation_group_files):
            raise ConfigError("The numbers of validation data files and validation group files do not match.")
    c.validation_gauc = opt(TRAIN, "validation_gauc", to_bool, c.validation_gauc)
    c.gauc_tolerance = opt(TRAIN, "gauc_tolerance", float, c.gauc_tolerance)
    if c.validation_gauc and not c.validation_group_files:
        raise ConfigError("validation_gauc needs validation_group_files.")
    if c.gauc_tolerance is not None and not c.validation_gauc:
        raise ConfigError("gauc_tolerance needs validation_gauc = true and validation_group_files.")
    vn = read(TRAIN, "validation_ndcg", required=False)
    if vn is not None:
        c.validation_ndcg = _cutoffs("validation_ndcg", [vn.strip()], 1)[0]
        if not c.validation_group_files:
            raise ConfigError("validation_ndcg needs validation_group_files.")
    c.ndcg_tolerance = opt(TRAIN, "ndcg_tolerance", float, c.ndcg_tolerance)
    if c.ndcg_tolerance is not None and c.validation_ndcg is None:
        raise ConfigError("ndcg_tolerance needs validation_ndcg and validation_group_files.")
    c.validation_ap = opt(TRAIN, "validation_ap", to_bool, c.validation_ap)
    c.ap_tolerance = opt(TRAIN, "ap_tolerance", float, c.ap_tolerance)
    if c.ap_tolerance is not None and not (c.validation_ap and c.validation_data_files):
        raise ConfigError("ap_tolerance needs validation_ap = true and validation_files.")

    pf = read_list(PREDICT, "predict_files", required=False)
    if pf is not None:
        c.predict_files = _expand(pf, base_dir)
    pgf = read_list(PREDICT, "predict_group_files", required=False)
    if pgf is not None:
        c.predict_group_files = _expand(pgf, base_dir)
        if len(c.predict_files) != len(c.predict_group_files):
            raise ConfigError("The numbers of predict files and predict group files do not match.")
    rc = read_list(PREDICT, "rank_cutoffs", required=False)
    if rc is not None:
        c.rank_cutoffs = _cutoffs("rank_cutoffs", rc, 4)
        if not c.predict_group_files:
            raise ConfigError("rank_cutoffs needs predict_group_files.")
    c.threshold_metrics = opt(PREDICT, "threshold_metrics", to_bool, c.threshold_metrics)
    for key in ("precision_targets", "recall_targets"):
        tg = read_list(PREDICT, key, required=False)
        if tg is not None:
            setattr(c, key, _targets(key, tg))
            c.threshold_metrics = True
    ai = read(PREDICT, "auc_interval", required=False)
    if ai is not None:
        try:
            c.auc_interval = float(ai)
        except ValueError:
            c.auc_interval = float("nan")
        if not 0.0 < c.auc_interval < 1.0:
            raise ConfigError(f"auc_interval must be a confidence level in (0, 1), got {ai.strip()}")
    bsf = read_list(PREDICT, "baseline_score_files", required=False)
    if bsf is not None:
        c.baseline_score_files = _expand(bsf, base_dir)
        if len(c.predict_files) != len(c.baseline_score_files):
            raise ConfigError("The numbers of predict files and baseline score files do not match.")

    c.mode = opt(DISTRIBUTED, "mode", lambda s: s.strip().lower(), c.mode)
    c.grad_reduce = opt(DISTRIBUTED, "grad_reduce", lambda s: s.strip().lower(), c.grad_reduce)
    c.comm_dtype = opt(DISTRIBUTED, "comm_dtype", lambda s: s.strip().lower(), c.comm_dtype)
    c.microbatches = opt(DISTRIBUTED, "microbatches", int, c.microbatches)
    c.prefetch_rows = opt(DISTRIBUTED, "prefetch_rows", lambda s: s.strip().lower(), c.prefetch_rows)
    c.overlap_grads = opt(DISTRIBUTED, "overlap_grads", lambda s: s.strip().lower(), c.overlap_grads)
    c.staleness = opt(DISTRIBUTED, "staleness", int, c.staleness)
    if c.loss_type in RANK_LOSSES and c.mode not in ("auto", "local"):
        raise ConfigError("loss_type = %s needs [Distributed] mode = local (or auto on one rank), got %s"
                          % (c.loss_type, c.mode))
    if c.comm_dtype not in ("auto", "storage", "fp32", "bf16"):
        raise ConfigError(f"[Distributed] comm_dtype must be auto, fp32 or bf16, got {c.comm_dtype}")
    if c.staleness not in (0, 1):
        raise ConfigError(f"[Distributed] staleness must be 0 or 1, got {c.staleness}")
    return c
