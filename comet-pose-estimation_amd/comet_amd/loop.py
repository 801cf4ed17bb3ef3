"""Loop-side callers of the COMET path (SURVEY §8(c) "Build counterpart of Python callers").

  process_spark_data2  train_util.py:637-667: batch dict -> (images, T_xyz, T_uvz, R, fl, pp, ratio,
                       seq_name, image_names, first_mask, R_matrix) on the device; default focal
                       cfg.default_focal_length and principal point (W/2, H/2) when absent
  train_or_eval_fn     train_eval_func_new_cp5.py:514-823, train and eval branches: keypoint
                       tracks from frame 0 (track_by_spsg: SuperPoint, plus the SIFT of
                       comet_amd.keypoints when train.track_by_sift is set), QuaternionCameras from the batch (597-606),
                       model(..., training) (under no_grad for eval), loss.mean(), the eval block's
                       pose metrics (comet_amd.metrics.pose_metrics), Stats, then for training
                       zero_grad -> accelerator.backward -> clip_grad_norm_ -> optimizer.step ->
                       lr_scheduler.step
  Stats                the subset of pytorch3d.implicitron Stats / train_util.VizStats the loop and
                       train_fn use (update / new_epoch / get_epoch_averages / status string /
                       gzip-JSON save and load); pytorch3d is not a dependency of this build
  CometAccelerator     the subset of accelerate.Accelerator train_e2epose2.py uses, on this build's
                       pieces: one process per GPU (RCCL), prepare() shards the train loader's
                       batches over ranks and attaches comet_amd.ddp.GradBucketer, backward() runs
                       the bucketed all-reduce, clip_grad_norm_ defers the scaling into the fused
                       AdamW kernel, mixed_precision "bf16" runs the model under
                       functional.precision(bf16), save_state / load_state write / read accelerate's
                       checkpoint files (comet_amd.checkpoint)
  build_dataset        train_util.py:335-347 for "AMD" / "AMD_eval": YTDataset behind DataLoaders
                       with the reference's loader settings, host stage in the workers and the
                       crop / resize on the device in this process (DeviceLoader)
  train_fn             train_e2epose2.py:45-186
  CsvLogger, test_fn   abl_ours.py:9-88, the evaluation entry point: eval loader (drop_last set
                       on its batch sampler), load_model_weights2, one eval pass of
                       train_or_eval_fn, one row in output_dir/test_results.csv
"""
import gzip
import json
import os
import random
import time

import numpy as np
import torch

from . import checkpoint as ckpt
from . import functional as F
from .models.utils import QuaternionCameras

TO_PLOT_METRICS = ("lr", "Auc_30", "Auc_10", "Auc_5", "Auc_3", "X_err", "Y_err", "Z_err", "Tx_mse", "Ty_mse",
                   "Tz_mse", "T_avg", "Racc_him_5", "Racc_him_10", "Racc_him_15", "R_avg", "Tacc_him_5",
                   "Tacc_him_10", "Tacc_him_15", "acc@5deg_x", "acc@5deg_y", "acc@5deg_z", "sec/it")  # train_util.py:96-121


def _get(cfg, path, default):
    cur = cfg
    for p in path.split("."):
        if isinstance(cur, dict) and p in cur:
            cur = cur[p]
        else:
            return default
    return cur


def process_spark_data2(batch, device, cfg):
    """train_util.py:637-667 (the `"spark" or ...` condition there is always true)."""
    images = batch["images"].to(device)
    translation = batch["T"].to(device)
    T_uvz = batch["T_uvz"].to(device) if "T_uvz" in batch else None
    rotation = batch["R"].to(device)
    ratio = batch["ratio"].to(device) if "ratio" in batch else None
    names = batch.get("seq_name")
    first_mask = batch.get("first_mask")
    image_names = batch.get("image_names")
    R_matrix_gt = batch.get("R_matrix")
    B, S = images.shape[:2]
    if "fl" in batch:
        fl = batch["fl"].to(device)
    else:
        fl = torch.ones(B, S, 2, device=device) * _get(cfg, "default_focal_length", 1745)
    if "pp" in batch:
        pp = batch["pp"].to(device)
    else:
        H, W = images.shape[-2:]
        pp = torch.tensor([W / 2, H / 2], device=device).expand(B, S, 2)
    return images, translation, T_uvz, rotation, fl, pp, ratio, names, image_names, first_mask, R_matrix_gt


# ------------------------------------------------------------------------------------------------
class AverageMeter:
    def __init__(self):
        self.reset()

    def reset(self):
        self.val, self.sum, self.count, self.history = 0.0, 0.0, 0, []

    def update(self, val, n=1, epoch=0):
        self.val = val
        self.sum += val * n
        self.count += n

    @property
    def avg(self):
        return self.sum / max(self.count, 1)

    def get_epoch_averages(self):
        return self.history


class Stats:
    """Per stat_set ("train" / "eval") running averages of `log_vars` over the current epoch
    (pytorch3d.implicitron.tools.stats.Stats semantics: `sec/it` = wall time since time_start over
    iterations; tensors are averaged to Python floats)."""

    def __init__(self, log_vars, epoch=-1):
        self.log_vars = list(log_vars)
        self.epoch = epoch
        self.it = {}
        self.stats = {}

    def hard_reset(self, epoch=-1):
        self.epoch = epoch
        self.it, self.stats = {}, {}

    def new_epoch(self):
        self.epoch += 1
        self.it, self.stats = {}, {}

    def update(self, preds, time_start=None, stat_set="train", freeze_iter=False):
        it = self.it.get(stat_set, -1) + (0 if freeze_iter else 1)
        self.it[stat_set] = it
        meters = self.stats.setdefault(stat_set, {})
        for k in self.log_vars:
            if k == "sec/it":
                if time_start is None:
                    continue
                v = (time.time() - time_start) / (it + 1)
                meters.setdefault(k, AverageMeter()).reset()
            elif k in preds and preds[k] is not None:
                v = preds[k]
            else:
                continue
            if torch.is_tensor(v):
                v = float(v.detach().float().mean())
            meters.setdefault(k, AverageMeter()).update(float(v))

    def get_epoch_averages(self):
        out = {}
        for ss, meters in self.stats.items():
            d = {k: m.avg for k, m in meters.items()}
            d["epoch"] = self.epoch
            d["it"] = self.it.get(ss, -1)
            out[ss] = d
        return out

    def get_status_string(self, stat_set="train", max_it=None):
        it = self.it.get(stat_set, -1)
        head = f"{stat_set} | epoch {self.epoch:3d} | it {it:5d}" + (f"/{max_it:5d}" if max_it else "")
        body = " | ".join(f"{k}: {m.avg:.4f}" for k, m in self.stats.get(stat_set, {}).items())
        return head + (" | " + body if body else "")

    def to_json(self):
        return json.dumps({"log_vars": self.log_vars, "epoch": self.epoch, "it": self.it,
                           "stats": {ss: {k: [m.val, m.sum, m.count] for k, m in ms.items()}
                                     for ss, ms in self.stats.items()}})

    def save(self, flpath):
        flpath = flpath if flpath.endswith(".jgz") else flpath + ".jgz"
        with gzip.open(flpath, "wt", encoding="utf-8") as f:
            f.write(self.to_json())

    @staticmethod
    def load(flpath):
        flpath = flpath if flpath.endswith(".jgz") else flpath + ".jgz"
        with gzip.open(flpath, "rt", encoding="utf-8") as f:
            d = json.loads(f.read())
        self = Stats(d["log_vars"], d["epoch"])
        self.it = d["it"]
        for ss, ms in d["stats"].items():
            for k, (val, sm, cnt) in ms.items():
                m = self.stats.setdefault(ss, {}).setdefault(k, AverageMeter())
                m.val, m.sum, m.count = val, sm, cnt
        return self


# ------------------------------------------------------------------------------------------------
class _BatchShard(torch.utils.data.Sampler):
    """Batch i of the wrapped batch sampler goes to rank i % world: accelerate's BatchSamplerShard
    without split_batches (accelerate==0.24.0, requirements.txt:1; installed by train_e2epose2.py:83's
    accelerator.prepare), restated here:

      * every rank yields batches only once all ranks have a full one (a round of `world` batches);
      * drop_last=True on the wrapped sampler: the last incomplete round is dropped;
      * even_batches=True (accelerate's default): the last round is completed -- and a short last
        batch filled -- with indices cycled from the start of the epoch (the first `world` batches),
        so every rank runs the same number of steps on full batches;
      * even_batches=False (train_e2epose2.py:47, abl_ours.py:28): the last round's batches go to the first ranks as they
        are, so the last ranks may run one batch fewer.
    `batch_size` / `drop_last` are read from the wrapped sampler (a plain list of batches: batch size
    None -- variable-length batches, cycled whole -- and drop_last False), as accelerate does.
    Pinned against the installed accelerate's implementation of the same algorithm
    (tests/test_checkpoint_cpu.py::test_batch_shard_matches_accelerate)."""

    def __init__(self, batch_sampler, rank, world, even_batches=True):
        self.bs, self.rank, self.world, self.even = batch_sampler, rank, world, even_batches
        self.batch_size = getattr(batch_sampler, "batch_size", None)
        self.drop_last = getattr(batch_sampler, "drop_last", False)

    def __len__(self):
        n = len(self.bs)
        if n % self.world == 0:
            return n // self.world
        length = n // self.world
        if self.drop_last:
            return length
        if self.even:
            return length + 1
        return length + 1 if self.rank < n % self.world else length

    def __iter__(self):
        W, R, bsz = self.world, self.rank, self.batch_size
        initial = []       # the first W batches' indices (flat), or the batches themselves (bsz None)
        pending = None     # this rank's batch of the current round, yielded once the round is full
        idx, batch = -1, []
        for idx, batch in enumerate(self.bs):
            if not self.drop_last and idx < W:
                if bsz is None:
                    initial.append(batch)
                else:
                    initial += list(batch)
            if idx % W == R:
                pending = batch
            if idx % W == W - 1 and (bsz is None or len(batch) == bsz):
                yield pending
                pending = None
        if self.drop_last or not initial:
            return
        if not self.even:
            if pending:
                yield pending
            return
        if pending and (bsz is None or len(pending) == bsz):
            yield pending
        need = W * bsz if bsz is not None else W
        while len(initial) < need:  # datasets smaller than one round
            initial += initial
        if bsz is None or len(batch) == bsz:  # the last batch seen was full (and yielded by its rank)
            batch = []
            idx += 1
        batch = list(batch)
        cyc = 0
        while idx % W != 0 or len(batch) > 0:
            if bsz is None:
                batch = initial[cyc]
                cyc += 1
            else:
                end = cyc + bsz - len(batch)
                batch = batch + initial[cyc:end]
                cyc = end
            if idx % W == R:
                yield batch
            batch = []
            idx += 1


class CometAccelerator:
    """accelerate.Accelerator subset of the reference's loops. Batches shard over ranks as
    accelerate's BatchSamplerShard does (_BatchShard): even_batches=True (accelerate's default)
    completes the last round with samples cycled from the epoch's start; even_batches=False (what
    every reference entry point passes: train_e2epose2.py:47, abl_ours.py:28, test_e2epose2.py:29)
    keeps the batches that do not fill every rank, so the last ranks may run one batch fewer."""

    def __init__(self, mixed_precision="no", device=None, bucket_mb=25, even_batches=True):
        import torch.distributed as dist
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        if device is None:
            local = int(os.environ.get("LOCAL_RANK", "0"))
            device = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.mixed_precision = mixed_precision
        self.bucket_mb = bucket_mb
        self.even_batches = even_batches
        self.ddp = None
        self._optimizer = None
        self.step = 0

    @property
    def is_main_process(self):
        return self.rank == 0

    @property
    def num_processes(self):
        return self.world

    def print(self, *a, **k):
        if self.is_main_process:
            print(*a, **k)

    def autocast(self):
        """mixed_precision "bf16": bf16 operands (accelerate's bf16 autocast); "no": fp32, as the
        reference runs without autocast (this build's process-wide default is bf16, so "no" must
        select fp32 explicitly)."""
        if self.mixed_precision == "bf16":
            return F.precision(torch.bfloat16)
        if self.mixed_precision == "fp16":
            raise ValueError("mixed_precision fp16 is not supported by this build (the reference config uses bf16)")
        return F.precision(torch.float32)

    def _shard(self, dl):
        if self.world == 1 or dl is None or getattr(dl, "batch_sampler", None) is None:
            return dl
        from .data import DeviceLoader
        inner = dl.loader if isinstance(dl, DeviceLoader) else dl
        kw = dict(batch_sampler=_BatchShard(inner.batch_sampler, self.rank, self.world, self.even_batches),
                  num_workers=inner.num_workers,
                  collate_fn=inner.collate_fn, pin_memory=inner.pin_memory, worker_init_fn=inner.worker_init_fn,
                  generator=inner.generator)
        if inner.num_workers > 0:
            kw.update(prefetch_factor=inner.prefetch_factor, persistent_workers=inner.persistent_workers)
        out = torch.utils.data.DataLoader(inner.dataset, **kw)
        return DeviceLoader(out, dl.device) if isinstance(dl, DeviceLoader) else out

    def prepare(self, model, dataloader=None, optimizer=None, lr_scheduler=None):
        """accelerator.prepare(model, dataloader, optimizer, lr_scheduler) (train_e2epose2.py:83):
        model to the device, train loader sharded over ranks, gradient buckets over the
        optimizer's params (the camera predictor) when world > 1. The optimizer's own clip is
        switched off: the loop clips through clip_grad_norm_ as the reference does. With world > 1
        every parameter and buffer is broadcast from rank 0 first (what DDP's _sync_module_states
        does when accelerate wraps the model): the ranks are seeded seed + rank, so their random
        inits differ, and load_model_weights always leaves pose_branch.fc2 at its init."""
        model = model.to(self.device)
        if self.world > 1:
            self.sync_module_states(model)
        if optimizer is not None and hasattr(optimizer, "max_norm"):
            optimizer.max_norm = None
        self._optimizer = optimizer
        if self.world > 1 and optimizer is not None:
            from .ddp import GradBucketer
            params = [p for g in optimizer.param_groups for p in g["params"]]
            self.ddp = GradBucketer(params, bucket_mb=self.bucket_mb)
        return model, self._shard(dataloader), optimizer, lr_scheduler

    @staticmethod
    @torch.no_grad()
    def sync_module_states(model, src=0):
        """Rank src's parameters and buffers to every rank, in state_dict order (one broadcast per
        tensor; runs once, at prepare)."""
        import torch.distributed as dist
        from . import functional as F
        params = list(model.parameters())
        for t in params + list(model.buffers()):
            dist.broadcast(t.data, src)
        # the broadcast writes through .data (no version bump): drop compute-dtype copies cast before it
        F.invalidate_weight_cache(params)

    def backward(self, loss):
        if self.ddp is not None:
            self.ddp.prepare_backward()
        loss.backward()
        if self.ddp is not None:
            self.ddp.finish_backward()

    def clip_grad_norm_(self, parameters, max_norm, optimizer=None):
        """-> total norm before clipping (device scalar). With a CometAdamW the scaling is applied
        by its next step(); otherwise torch.nn.utils.clip_grad_norm_."""
        opt = optimizer if optimizer is not None else getattr(self, "_optimizer", None)
        if opt is not None and hasattr(opt, "clip_grad_norm_"):
            return opt.clip_grad_norm_(max_norm)
        return torch.nn.utils.clip_grad_norm_(list(parameters), max_norm)

    def save_state(self, output_dir, model, optimizer=None, lr_scheduler=None, safe_serialization=False):
        if safe_serialization:
            raise ValueError("safe_serialization=True is not used by the reference (train_e2epose2.py:160)")
        return ckpt.save_state(output_dir, model, optimizer, lr_scheduler, step=self.step, process_index=self.rank)

    def load_state(self, input_dir, model, optimizer=None, lr_scheduler=None):
        self.step = ckpt.load_state(input_dir, model, optimizer, lr_scheduler, process_index=self.rank,
                                    device=self.device)


# ------------------------------------------------------------------------------------------------
def _keypoint_init(cfg, device):
    from .keypoints import SuperPoint
    return SuperPoint(max_num_keypoints=_get(cfg, "train.track_num", 512), detection_threshold=0.005).to(device).eval()


def _sift_init(cfg, device):
    """The reference's second detector, lightglue.SIFT(max_num_keypoints=track_num)
    (train_eval_func_new_cp5.py:529-531), built only when train.track_by_sift is true."""
    if not _get(cfg, "train.track_by_sift", False):
        return None
    from .keypoints import SIFT
    return SIFT(max_num_keypoints=_get(cfg, "train.track_num", 512)).to(device).eval()


def train_or_eval_fn(model, dataloader, cfg, optimizer, stats, accelerator, lr_scheduler, training=True, epoch=-1,
                     sp=None):
    """train_eval_func_new_cp5.py:514-823 (visualisation / demo-JSON branches excluded).
    `sp`: a SuperPoint detector to reuse across calls (built here when track_by_spsg is set)."""
    model.train() if training else model.eval()
    time_start = time.time()
    max_it = len(dataloader)
    dev = accelerator.device
    spsg = bool(_get(cfg, "enable_track", True) and _get(cfg, "track_by_spsg", False)
                and not _get(cfg, "labor_input_traj", False))
    if spsg and sp is None:
        sp = _keypoint_init(cfg, dev)
    sift = _sift_init(cfg, dev) if spsg else None
    acc5 = [0.0, 0.0, 0.0]
    for step, batch in enumerate(dataloader):
        (images, T_xyz, T_uvz, rotation, fl, pp, ratio, sel_first_name, image_names, mask,
         R_matrix_gt) = process_spark_data2(batch, dev, cfg)
        bbb, ttt = images.shape[:2]
        if spsg:
            from .keypoints import keypoint_tracks
            tracks, tracks_visibility = keypoint_tracks(sp, images, mask.to(dev).bool(), _get(cfg, "train.track_num", 512),
                                                        sift=sift, min_required=256, names=sel_first_name)
        else:
            tracks, tracks_visibility = None, None
        gt_cameras = None
        if rotation is not None:
            gt_cameras = QuaternionCameras(focal_length=fl.reshape(-1, 2), principal_point=pp.reshape(-1, 2),
                                           R=rotation.reshape(-1, 4), T_uvz=T_uvz.reshape(-1, 3),
                                           T=T_xyz.reshape(-1, 3), ratio=ratio, device=dev)
        with accelerator.autocast():
            if training:
                predictions = model(images, gt_cameras=gt_cameras, training=True, tracks=tracks,
                                    tracks_visibility=tracks_visibility)
                predictions["loss"] = predictions["loss"].mean()
                loss = predictions["loss"]
            else:
                with torch.no_grad():
                    predictions = model(images, gt_cameras=gt_cameras, training=False, tracks=tracks,
                                        tracks_visibility=tracks_visibility)
                predictions["loss"] = predictions["loss"].mean()
        if "gt_pose_enc" in predictions and predictions["gt_pose_enc"] is not None:
            from .metrics import pose_metrics
            with torch.no_grad():
                predictions.update(pose_metrics(predictions, gt_cameras, bbb, dev))
            for i, k in enumerate(("acc@5deg_x", "acc@5deg_y", "acc@5deg_z")):
                acc5[i] += float(predictions[k])
        ss = "train" if training else "eval"
        stats.update(predictions, time_start=time_start, stat_set=ss)
        pi = _get(cfg, "train.print_interval" if training else "train.eval_print_interval", 50)
        if pi and step % pi == 0:
            accelerator.print(stats.get_status_string(stat_set=ss, max_it=max_it))
        if training:
            optimizer.zero_grad()
            accelerator.backward(loss)
            clip = _get(cfg, "train.clip_grad", 1.0)
            if clip > 0:
                accelerator.clip_grad_norm_(model.parameters(), clip, optimizer=optimizer)
            optimizer.step()
            lr_scheduler.step()
            accelerator.step += 1
    n = max(len(dataloader), 1)
    accelerator.print("x", "y", "z", acc5[0] / n, acc5[1] / n, acc5[2] / n)
    return True


# ------------------------------------------------------------------------------------------------
def seed_worker(worker_id):
    """train_util.py:803-806."""
    s = torch.initial_seed() % 2 ** 32
    np.random.seed(s)
    random.seed(s)


def set_seed_and_print(seed, device_specific=True):
    """train_util.py:1847-1849 (accelerate.utils.set_seed(seed, device_specific=True): seed +
    process index for python, numpy and torch)."""
    import torch.distributed as dist
    if device_specific and dist.is_initialized():
        seed += dist.get_rank()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    print(f"----------Seed is set to {np.random.get_state()[1][0]} now----------")


def build_dataset(cfg, data_root=None, device="cuda"):
    """train_util.py:335-347, 808-926 for the YT datasets ("AMD": train + eval loaders,
    "AMD_eval": eval loader only). data_root: the directory holding AMD_train / AMD_eval
    (the reference's comet/datasets/AMD; cfg.data_root or $COMET_DATA_ROOT here)."""
    from torch.utils.data import ConcatDataset, DataLoader, SequentialSampler
    from .data import DeviceLoader, YTDataset, collate_host
    name = _get(cfg, "train.dataset", "AMD")
    if name not in ("AMD", "AMD_eval"):
        raise ValueError("Dataset Not Implemented")
    root = data_root or _get(cfg, "data_root", None) or os.environ.get("COMET_DATA_ROOT")
    if root is None:
        raise ValueError("build_dataset: give data_root (the reference's comet/datasets/AMD directory)")
    size = int(_get(cfg, "train.img_size", 512))
    nw = int(_get(cfg, "train.num_workers", 8))
    mk = lambda split, augs: YTDataset(os.path.join(root, "AMD_train" if split == "train" else "AMD_eval"),  # noqa: E731
                                       crop_size=[size, size], seq_len=int(_get(cfg, "seqlen", 16)), use_augs=augs,
                                       split=split, device=device)
    eval_dataset = mk("valid", False)
    eval_loader = DeviceLoader(DataLoader(eval_dataset, sampler=SequentialSampler(eval_dataset), batch_size=1,
                                          num_workers=nw, pin_memory=True, persistent_workers=nw > 0,
                                          collate_fn=collate_host), device)
    if name == "AMD_eval":
        return None, None, None, eval_loader
    train_dataset = ConcatDataset([mk("train", True)] * int(_get(cfg, "repeat_kub", 1)))
    g = torch.Generator()
    g.manual_seed(0)
    kw = dict(prefetch_factor=1) if nw > 0 else {}
    train_loader = DeviceLoader(DataLoader(train_dataset, batch_size=int(_get(cfg, "batch_size", 1)), shuffle=True,
                                           persistent_workers=False, num_workers=nw, worker_init_fn=seed_worker,
                                           generator=g, pin_memory=True, drop_last=True, collate_fn=collate_host, **kw),
                                device)
    return train_dataset, eval_dataset, train_loader, eval_loader


def train_fn(cfg, data_root=None, eval_only=True, csv_log=True):
    """train_e2epose2.py:45-186. As written, the reference returns right after the first
    evaluation (train_e2epose2.py:131, `return` before the epoch loop); `eval_only=True` keeps that
    behaviour, `eval_only=False` runs the epoch loop that follows it (train, ckpt_DDDDDD every
    ckpt_interval epochs, eval every eval_interval epochs, a final checkpoint)."""
    from .config import instantiate
    from .train import build_optimizer
    # train_e2epose2.py:47: Accelerator(even_batches=False, ...) -- with the train loader's
    # drop_last=True the shards are the same either way; a loader without it keeps its tail batches
    acc = CometAccelerator(mixed_precision=_get(cfg, "mixed_precision", "no"), even_batches=False)
    set_seed_and_print(int(_get(cfg, "seed", 0)))
    exp_dir = _get(cfg, "exp_dir", "exp")
    logger = None
    if acc.is_main_process and csv_log:
        import csv
        os.makedirs(exp_dir, exist_ok=True)
        path = os.path.join(exp_dir, "train_eval_stats.csv")
        fields = ["epoch", "it", "mode"] + list(TO_PLOT_METRICS) + ["lr"]
        if not os.path.exists(path):
            with open(path, "w", newline="") as f:
                csv.DictWriter(f, fieldnames=fields).writeheader()

        def logger(row):
            with open(path, "a", newline="") as f:
                csv.DictWriter(f, fieldnames=fields).writerow(row)
    dataset, eval_dataset, dataloader, eval_dataloader = build_dataset(cfg, data_root, acc.device)
    model = instantiate(cfg["MODEL"], _recursive_=False, cfg=cfg).to(acc.device)
    optimizer, lr_scheduler = build_optimizer(cfg, model, dataloader if dataloader is not None else 1)
    resume = _get(cfg, "train.resume_ckpt", "")
    if resume:
        acc.print(f"Loading ckpt from {resume}")
        model = ckpt.load_model_weights(model, resume, acc.device, _get(cfg, "relax_load", False))
    model, dataloader, optimizer, lr_scheduler = acc.prepare(model, dataloader, optimizer, lr_scheduler)
    start_epoch = 0
    stats = Stats(TO_PLOT_METRICS)
    if _get(cfg, "train.auto_resume", False):
        last = ckpt.find_last_checkpoint(exp_dir)
        ep, start = ckpt.resume_epoch(last)
        if last is not None and ep > 0:
            acc.print(f"Loading ckpt from {last}")
            acc.load_state(last, model, optimizer, lr_scheduler)
            start_epoch = start
            try:
                stats = Stats.load(os.path.join(last, "train_stats.jgz"))
            except (OSError, ValueError, KeyError):
                stats.hard_reset(epoch=start_epoch)

    def run_eval(epoch):
        lr = lr_scheduler.get_last_lr()[0]
        train_or_eval_fn(model, eval_dataloader, cfg, optimizer, stats, acc, lr_scheduler, training=False, epoch=epoch)
        stats.update({"lr": lr}, stat_set="eval")
        d = stats.get_epoch_averages()["eval"]
        if logger:
            logger({"epoch": d["epoch"], "it": d["it"], "mode": "eval", **{k: d.get(k, "") for k in TO_PLOT_METRICS}})

    run_eval(start_epoch - 1)
    if eval_only:
        return
    epoch = start_epoch
    for epoch in range(start_epoch, int(_get(cfg, "train.epochs", 1))):
        stats.new_epoch()
        set_seed_and_print(int(_get(cfg, "seed", 0)) + epoch * 1000)
        train_or_eval_fn(model, dataloader, cfg, optimizer, stats, acc, lr_scheduler, training=True, epoch=epoch)
        if acc.is_main_process:
            stats.update({"lr": lr_scheduler.get_last_lr()[0]}, stat_set="train")
            d = stats.get_epoch_averages()["train"]
            if logger:
                logger({"epoch": d["epoch"], "it": d["it"], "mode": "train", "lr": d.get("lr", ""),
                        **{k: d.get(k, "") for k in TO_PLOT_METRICS if k != "lr"}})
        if epoch != 0 and epoch % int(_get(cfg, "train.ckpt_interval", 1)) == 0 and acc.is_main_process:
            path = ckpt.checkpoint_path(exp_dir, epoch)
            acc.save_state(path, model, optimizer, lr_scheduler)
            ckpt.save_tdict(path, epoch, cfg)
            stats.save(os.path.join(path, "train_stats.jgz"))
        if epoch != 0 and epoch % int(_get(cfg, "train.eval_interval", 1)) == 0:
            run_eval(epoch)
    acc.save_state(ckpt.checkpoint_path(exp_dir, epoch), model, optimizer, lr_scheduler)
    return True


# ------------------------------------------------------------------------------------------------
def sequence_stream(seq_dir):
    """One YTDataset sequence directory (frames/frame_*, Mask/mask_*) as a stream: -> (iterator over
    every frame in order, uint8 [H, W, 3] host arrays; the sequence's square crop box, computed as
    YTDataset.load_host does but over all frames). Host only."""
    from PIL import Image
    from .data import make_bbox_square, mask_bbox
    fdir, mdir = os.path.join(seq_dir, "frames"), os.path.join(seq_dir, "Mask")
    names = sorted(f for f in os.listdir(fdir) if f.startswith("frame_"))
    boxes = [mask_bbox(np.array(Image.open(os.path.join(mdir, m)).convert("L"), dtype=np.uint8))
             for m in sorted(f for f in os.listdir(mdir) if f.startswith("mask_"))]
    xmins, ymins, xmaxs, ymaxs = zip(*boxes)
    bbox = np.array([min(xmins), min(ymins), max(xmaxs), max(ymaxs)], dtype=np.float64)
    size = np.max([bbox[2] - bbox[0], bbox[3] - bbox[1]])
    bbox = bbox + np.array([-1.0, -1.0, 1.0, 1.0]) * (size * 0.15)
    box = tuple(int(v) for v in make_bbox_square(bbox, size * 1.3))
    return (np.asarray(Image.open(os.path.join(fdir, n)).convert("RGB")) for n in names), box


STREAM_FIELDS = ("frame_index", "newest_frame", "du", "dv", "dd", "qw", "qx", "qy", "qz", "hop_ms")
# cfg.stream.fuse: one row per frame whose fused pose is final, these columns after the hop's own
FUSE_FIELDS = ("fused_frame", "fused_qw", "fused_qx", "fused_qy", "fused_qz", "fused_tx", "fused_ty", "fused_tz",
               "fused_count", "rot_spread", "spread_u", "spread_v", "spread_z")


def _stream_fuse(cfg, anchor):
    """cfg.stream.fuse / fuse_weight -> (fuse, fuse_weight, anchor, CSV fields). Without an anchor the
    fused poses are relative to the stream's first frame: identity rotation at the principal point,
    depth 1, of cfg.stream.dataset (default "AMD") with cfg.stream.ratio (default 1.0)."""
    fuse = bool(_get(cfg, "stream.fuse", False))
    if not fuse:
        return False, None, anchor, STREAM_FIELDS
    if anchor is None:
        from .models.utils import INTRINSICS
        dataset = _get(cfg, "stream.dataset", "AMD")
        fx, _, cx, cy = INTRINSICS[dataset]
        anchor = ([1.0, 0.0, 0.0, 0.0], [cx, cy, 1.0], fx, float(_get(cfg, "stream.ratio", 1.0)), dataset)
    return True, _get(cfg, "stream.fuse_weight", None), anchor, STREAM_FIELDS + FUSE_FIELDS


# cfg.stream.carry: these columns after all others, per hop
CARRY_FIELDS = ("survivors", "born", "padded")


def _stream_carry(cfg, sp, sift, candidate_fn, device):
    """cfg.stream.carry (default false) / carry_tracks (default cfg.train.track_num) / carry_cell (8) /
    carry_border (0) / carry_min_score (required) / detect_every (1) -> the carry keywords of PoseStream
    / StreamPool ({} with carry off). candidate_fn: default keypoint_candidates of the detectors."""
    if not _get(cfg, "stream.carry", False):
        if _get(cfg, "stream.warm", False):
            raise ValueError("cfg.stream.warm needs cfg.stream.carry: the warm start follows the carried tracks")
        return {}
    from .stream import keypoint_candidates
    if candidate_fn is None:
        candidate_fn = keypoint_candidates(sp if sp is not None else _keypoint_init(cfg, device), sift)
    kw = dict(carry=True, carry_tracks=int(_get(cfg, "stream.carry_tracks", _get(cfg, "train.track_num", 512))),
              carry_cell=int(_get(cfg, "stream.carry_cell", 8)), carry_border=int(_get(cfg, "stream.carry_border", 0)),
              carry_min_score=_get(cfg, "stream.carry_min_score", None),
              detect_every=int(_get(cfg, "stream.detect_every", 1)), candidate_fn=candidate_fn)
    if _get(cfg, "stream.warm", False):
        kw.update(warm=True, warm_mode=_get(cfg, "stream.warm_mode", "hold"), warm_iters=_get(cfg, "stream.warm_iters", None))
    return kw


# cfg.stream.warm: this column after the carry columns, per hop
WARM_FIELDS = ("warm",)


def _carry_fields(carry):
    """The trailing CSV columns of the keywords _stream_carry returned."""
    if not carry:
        return ()
    return CARRY_FIELDS + (WARM_FIELDS if carry.get("warm") else ())


# cfg.stream.landmarks: a second CSV per sequence, one row per valid live landmark of the last hop
LANDMARK_FIELDS = ("track_id", "x", "y", "z", "n_obs")


def _stream_archive(cfg):
    """cfg.stream.lm_archive (default 0: off) / reid_px (required with lm_archive: nothing here derives one) /
    reid_min_cos (0.5, a stated value, not a tuned one) / lm_arch_min_obs (null: lm_min_obs) -> the archive
    keywords of PoseStream / StreamPool ({} with the archive off)."""
    cap = int(_get(cfg, "stream.lm_archive", 0))
    if not cap:
        return {}
    px = _get(cfg, "stream.reid_px", None)
    if px is None:
        raise ValueError("cfg.stream.lm_archive needs cfg.stream.reid_px, the re-identification gate in pixels")
    obs = _get(cfg, "stream.lm_arch_min_obs", None)
    return dict(lm_archive=cap, reid_px=float(px), reid_min_cos=float(_get(cfg, "stream.reid_min_cos", 0.5)),
                lm_arch_min_obs=None if obs is None else int(obs))


def _stream_landmarks(cfg, fuse, carry):
    """cfg.stream.landmarks (default false) / lm_min_obs (3) / lm_min_pivot (1e-8, a guard, not a tuned
    value) / lm_weight (null or "score") / lm_gate_px (null: no gate) / lm_inverse_rotation (0) -> the
    landmark keywords of PoseStream / StreamPool without the intrinsics ({} with landmarks off), which
    depend on the sequence's box (_track_intr). fuse, carry: what _stream_fuse / _stream_carry returned."""
    if not _get(cfg, "stream.landmarks", False):
        if int(_get(cfg, "stream.lm_archive", 0)):
            raise ValueError("cfg.stream.lm_archive needs cfg.stream.landmarks: the archive keeps the landmarks of dead "
                             "tracks")
        return {}
    if not fuse or not carry:
        raise ValueError("cfg.stream.landmarks needs cfg.stream.fuse and cfg.stream.carry: a landmark is a carried "
                         "track triangulated from the fused poses")
    gate = _get(cfg, "stream.lm_gate_px", None)
    return dict(_stream_archive(cfg), landmarks=True, lm_min_obs=int(_get(cfg, "stream.lm_min_obs", 3)),
                lm_min_pivot=float(_get(cfg, "stream.lm_min_pivot", 1e-8)), lm_weight=_get(cfg, "stream.lm_weight", None),
                lm_gate_px=None if gate is None else float(gate),
                lm_inverse_rotation=int(_get(cfg, "stream.lm_inverse_rotation", 0)))


# cfg.stream.pnp: a third CSV per sequence, one row per hop for the frame that becomes the next window's first
PNP_FIELDS = ("hop", "frame", "state", "inliers", "rms_px", "qw", "qx", "qy", "qz", "tx", "ty", "tz")


def _stream_pnp(cfg, lm):
    """cfg.stream.pnp (default false) / pnp_iters (4, a stated number of steps, not a tuned value) /
    pnp_huber_px (required with pnp: nothing here derives one) / pnp_min_pts (6) / pnp_weight (0: report
    only) -> the PnP keywords of PoseStream / StreamPool ({} with pnp off). lm: what _stream_landmarks
    returned."""
    if not _get(cfg, "stream.pnp", False):
        return {}
    if not lm:
        raise ValueError("cfg.stream.pnp needs cfg.stream.landmarks: a frame is posed against the landmark map")
    huber = _get(cfg, "stream.pnp_huber_px", None)
    if huber is None:
        raise ValueError("cfg.stream.pnp needs cfg.stream.pnp_huber_px, the Huber threshold in pixels")
    return dict(pnp=True, pnp_iters=int(_get(cfg, "stream.pnp_iters", 4)), pnp_huber_px=float(huber),
                pnp_min_pts=int(_get(cfg, "stream.pnp_min_pts", 6)), pnp_weight=float(_get(cfg, "stream.pnp_weight", 0.0)))


def pnp_csv(csv_path):
    """The path of the PnP CSV that goes with the hop CSV csv_path: <stem>_pnp.csv."""
    stem, ext = os.path.splitext(csv_path)
    return stem + "_pnp" + ext


def _log_pnp(logger, hop, r, stride):
    """One row of the PnP CSV (PNP_FIELDS): window position `stride` of the hop's StreamResult, the frame
    that becomes the next window's first (the input pose, with state != 1, where nothing was solved)."""
    i = int(stride)
    vals = [hop, r.frame_index + i, int(r.pnp_state[i]), int(r.pnp_inliers[i]), float(r.pnp_rms_px[i])]
    logger.log(dict(zip(PNP_FIELDS, vals + r.pnp_R[i].double().tolist() + r.pnp_T[i].double().tolist())))


# cfg.stream.motion: one more CSV per sequence, one row per hop
MOTION_FIELDS = ("hop", "frame", "state", "frames", "wx", "wy", "wz", "vx", "vy", "vz", "qw", "qx", "qy", "qz", "tx", "ty",
                 "tz", "rot_rms", "trans_rms_x", "trans_rms_y", "trans_rms_z", "innov_rot", "innov_trans")


def _stream_motion(cfg, fuse):
    """cfg.stream.motion (default false) / motion_len (16) / motion_min_frames (3) / motion_iters (2) /
    motion_horizon (1) / motion_max_angle (2.0 rad) / motion_inverse_rotation (0), all stated values, not tuned
    ones -> the motion keywords of PoseStream / StreamPool ({} with motion off)."""
    if not _get(cfg, "stream.motion", False):
        return {}
    if not fuse:
        raise ValueError("cfg.stream.motion needs cfg.stream.fuse: the motion is fitted to the final fused poses")
    return dict(motion=True, motion_len=int(_get(cfg, "stream.motion_len", 16)),
                motion_min_frames=int(_get(cfg, "stream.motion_min_frames", 3)),
                motion_iters=int(_get(cfg, "stream.motion_iters", 2)),
                motion_horizon=int(_get(cfg, "stream.motion_horizon", 1)),
                motion_max_angle=float(_get(cfg, "stream.motion_max_angle", 2.0)),
                motion_inverse_rotation=int(_get(cfg, "stream.motion_inverse_rotation", 0)))


def motion_csv(csv_path):
    """The path of the motion CSV that goes with the hop CSV csv_path: <stem>_motion.csv."""
    stem, ext = os.path.splitext(csv_path)
    return stem + "_motion" + ext


def _log_motion(logger, hop, r):
    """One row of the motion CSV (MOTION_FIELDS) for a hop's StreamResult: `frame` is the newest frame whose
    fused pose is final, where q / t (the fitted pose) and the rates (rad / frame, per frame) apply;
    innov_* is the innovation on the frame after it (+inf, like the rms columns, where state != 1)."""
    vals = [hop, r.frame_index + r.final - 1, int(r.motion_state), int(r.motion_frames)]
    vals += r.motion_omega.tolist() + r.motion_vel.tolist() + r.motion_q0.tolist() + r.motion_t0.tolist()
    vals += [float(r.motion_rot_rms)] + r.motion_trans_rms.double().tolist()
    vals += [float(r.motion_innov_rot[0]), float(r.motion_innov_trans[0])]
    logger.log(dict(zip(MOTION_FIELDS, vals)))


def _track_intr(dataset, box, size):
    """(fx, fy, cx, cy) of the pixels the tracks of a sequence live in: the dataset's intrinsics mapped
    into the crop `box` resized to size x size, the frames stream_eval pushes."""
    from .data import crop_intrinsics
    from .models.utils import INTRINSICS
    return crop_intrinsics(INTRINSICS[dataset], box, size)


def landmarks_csv(csv_path):
    """The path of the landmark CSV that goes with the hop CSV csv_path: <stem>_landmarks.csv."""
    stem, ext = os.path.splitext(csv_path)
    return stem + "_landmarks" + ext


def _log_landmarks(csv_path, lm, stream=0):
    """LandmarkMap.snapshot(stream), the valid live landmarks of the stream's last hop, as
    landmarks_csv(csv_path): one row per landmark (LANDMARK_FIELDS; x, y, z in the body frame), the
    header alone when there is none. -> number of rows."""
    logger = CsvLogger(landmarks_csv(csv_path), LANDMARK_FIELDS)
    ids, X, n_obs = lm.snapshot(stream)
    rows = torch.cat([ids.double()[:, None], X.double(), n_obs.double()[:, None]], 1).tolist()
    for i, x, y, z, k in rows:
        logger.log(dict(zip(LANDMARK_FIELDS, (int(i), x, y, z, int(k)))))
    return len(rows)


def archive_csv(csv_path):
    """The path of the archive CSV that goes with the hop CSV csv_path: <stem>_archive.csv."""
    stem, ext = os.path.splitext(csv_path)
    return stem + "_archive" + ext


def _log_archive(csv_path, lm, stream=0):
    """LandmarkMap.archive_snapshot(stream), the landmarks of dead tracks the stream's archive holds, as
    archive_csv(csv_path): one row per entry in use, with the landmark CSV's fields (id = the landmark's
    identity), the header alone when there is none. -> number of rows."""
    logger = CsvLogger(archive_csv(csv_path), LANDMARK_FIELDS)
    ids, X, n_obs = lm.archive_snapshot(stream)
    rows = torch.cat([ids.double()[:, None], X.double(), n_obs.double()[:, None]], 1).tolist()
    for i, x, y, z, k in rows:
        logger.log(dict(zip(LANDMARK_FIELDS, (int(i), x, y, z, int(k)))))
    return len(rows)


def _carry_counts(r):
    """(survivors, born, padded) of a carried StreamResult, from track_src (ops.CarryOut)."""
    src = r.track_src.tolist()
    survivors = sum(1 for j, v in enumerate(src) if v == j)
    born = sum(1 for v in src if -1 - 65536 < v < 0)
    return survivors, born, len(src) - survivors - born


def _fused_rows(r, positions):
    """The FUSE_FIELDS columns of the window positions `positions` of a fused StreamResult."""
    cols = torch.cat([r.fused_R.double(), r.fused_T, r.fused_count[:, None].double(), r.rot_spread[:, None].double(),
                      r.trans_spread.double()], 1).tolist()
    rows = []
    for i in positions:
        c = cols[i]
        rows.append(dict(zip(FUSE_FIELDS, [r.frame_index + i] + c[:7] + [int(c[7])] + c[8:])))
    return rows


def _log_hop(logger, fields, r, window, ms, last=None):
    """One hop's CSV rows. Without fusion: one row. With it: one row per final frame of the hop (the
    hop's own columns repeated). last: the hop's row dict again, for the flush at the end of the
    stream (the frames of the last window that no later hop made final)."""
    if last is None:
        enc = r.pred_pose_enc[-1].tolist()  # (synchronises: the events are complete after it)
        row = dict(zip(STREAM_FIELDS, [r.frame_index, r.frame_index + window - 1] + enc + [ms]))
        if r.track_src is not None:
            row.update(zip(CARRY_FIELDS, _carry_counts(r)))
        if r.track_warm is not None:  # slots whose coarse tracker started warm (carried, or a pad of a carried slot)
            row[WARM_FIELDS[0]] = int((r.track_warm > 0).sum())
        positions = range(r.final) if r.final is not None else None
    else:
        row, positions = last, range(r.final, window)
    if positions is None:
        logger.log(row)
    else:
        for extra in _fused_rows(r, positions):
            logger.log({**row, **extra})
    return row


def stream_eval(model, frames_iter, cfg, box, csv_path, sp=None, sift=None, query_points=None, device="cuda",
                anchor=None, candidate_fn=None):
    """Online evaluation of one long sequence (opt-in: cfg.stream.enable must be true; train_fn /
    test_fn never call it). frames_iter yields uint8 [H, W, 3] frames in order (sequence_stream);
    each is cropped to `box` and resized / normalised on the device (crop_resize_normalize, the
    loader's pixel path) and pushed into a comet_amd.stream.PoseStream of cfg.stream.window
    (default cfg.seqlen) frames, cfg.stream.stride (1) and cfg.stream.capacity (window). Query points:
    `query_points` [N, 2] for every window, else SuperPoint (+ SIFT) keypoints of each window's first
    frame. One CSV row per hop: the window's first frame, its newest frame, the newest frame's pose
    encoding relative to the first (du, dv, dd, quaternion) and the time of the push that completed
    the hop (per-frame stages of the new frame + the hop), from device events. -> number of hops.
    anchor: the 5-tuple PoseStream takes. cfg.stream.fuse (default false; cfg.stream.fuse_weight: null
    or "score") turns pose fusion on: the CSV gains the FUSE_FIELDS columns, one row per frame whose
    fused pose is final (the first `stride` frames of each hop), and at the end of the stream one
    flush writes the remaining frames of the last window. With fusion off the CSV is what it was.
    cfg.stream.carry (default false; with carry_cell, carry_border, carry_tracks, detect_every and the
    required carry_min_score) turns track carry on (PoseStream carry=True): the queries come from the
    carried tracks and candidate_fn (default: keypoint_candidates of the detectors), query_points must
    be None, and the CSV gains the trailing columns survivors, born, padded. Off: the CSV is what it was.
    cfg.stream.warm (default false; needs cfg.stream.carry; with warm_mode "hold" / "velocity" and warm_iters,
    default cfg.track_trainit) starts the coarse tracker of every hop but the first from the previous
    window's tracks (PoseStream warm=True); the CSV gains a last column warm, the slots that started so.
    cfg.stream.landmarks (default false; needs fuse and carry; with lm_min_obs, lm_min_pivot, lm_weight,
    lm_gate_px and lm_inverse_rotation) turns the landmark map on (PoseStream landmarks=True) with the
    intrinsics of the anchor's dataset mapped into `box` (data.crop_intrinsics); the hop CSV is what it
    was, and at the end of the stream landmarks_csv(csv_path) takes the final snapshot, one row per valid
    live landmark (LANDMARK_FIELDS). cfg.stream.lm_archive = C > 0 (with reid_px, required, reid_min_cos and
    lm_arch_min_obs) turns the landmark archive on (PoseStream lm_archive): archive_csv(csv_path) then takes
    LandmarkMap.archive_snapshot at the end, with the same fields; with it off (the default) the hop CSV and
    the landmark CSV are what they were and no archive CSV is written.
    cfg.stream.motion (default false; needs fuse; with motion_len, motion_min_frames, motion_iters,
    motion_horizon, motion_max_angle and motion_inverse_rotation) turns the motion estimate on (PoseStream
    motion=True); the hop CSV is what it was, and motion_csv(csv_path) takes one row per hop (MOTION_FIELDS)."""
    from .data import crop_resize_normalize
    from .stream import PoseStream, keypoint_query
    if not _get(cfg, "stream.enable", False):
        raise ValueError("stream_eval is opt-in: set cfg.stream.enable")
    model.eval()
    window = int(_get(cfg, "stream.window", _get(cfg, "seqlen", 16)))
    size = int(_get(cfg, "train.img_size", 512))
    query_fn = None
    carry = _stream_carry(cfg, sp, sift, candidate_fn, device)
    if query_points is None and not carry:
        sp = sp if sp is not None else _keypoint_init(cfg, device)
        query_fn = keypoint_query(sp, sift=sift, track_num=_get(cfg, "train.track_num", 512))
    mp = _get(cfg, "mixed_precision", "no")
    fuse, fuse_weight, anchor, fields = _stream_fuse(cfg, anchor)
    lm = _stream_landmarks(cfg, fuse, carry)
    pnp = _stream_pnp(cfg, lm)
    motion = _stream_motion(cfg, fuse)
    if lm:
        lm["track_intr"] = _track_intr(anchor[4], box, size)
    stream = PoseStream(model, window=window, stride=int(_get(cfg, "stream.stride", 1)),
                        capacity=_get(cfg, "stream.capacity", None), query_fn=query_fn, anchor=anchor,
                        precision=torch.bfloat16 if mp == "bf16" else torch.float32, fuse=fuse, fuse_weight=fuse_weight,
                        **carry, **lm, **pnp, **motion)
    if carry:
        fields = tuple(fields) + _carry_fields(carry)
    logger = CsvLogger(csv_path, fields)
    pnp_logger = CsvLogger(pnp_csv(csv_path), PNP_FIELDS) if pnp else None
    motion_logger = CsvLogger(motion_csv(csv_path), MOTION_FIELDS) if motion else None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hops, last = 0, None
    for frame in frames_iter:
        up = torch.as_tensor(frame)[None].to(device)
        e0.record()
        results = stream.push(crop_resize_normalize(up, box, (size, size))[0], query_points=query_points)
        e1.record()
        for r in results:
            e1.synchronize()
            last = (r, _log_hop(logger, fields, r, window, e0.elapsed_time(e1)))
            if pnp:
                _log_pnp(pnp_logger, hops, r, stream.landmark_map.stride)
            if motion:
                _log_motion(motion_logger, hops, r)
            hops += 1
    if fuse and last is not None:
        _log_hop(logger, fields, last[0], window, None, last=last[1])
    if lm:
        _log_landmarks(csv_path, stream.landmark_map)
        if lm.get("lm_archive"):
            _log_archive(csv_path, stream.landmark_map)
    return hops


def stream_eval_pool(model, sequences, cfg, csv_dir, sp=None, sift=None, query_points=None, device="cuda",
                     anchors=None, candidate_fn=None):
    """stream_eval for several sequences at a time (opt-in: cfg.stream.enable). `sequences` is an
    iterable of (name, frames_iter, box), each as stream_eval takes them; cfg.stream.streams
    (default 4) streams of one comet_amd.stream.StreamPool run side by side. Every free stream takes
    the next sequence (reset(stream), then its frames); one push carries one frame of every running
    sequence, and when a sequence ends the pool goes on with the streams that remain. One CSV per
    sequence, csv_dir/<name>.csv, with the rows stream_eval writes; hop_ms is the time of the push
    that completed the hop (the frames of all running streams and all hops due in it), from device
    events. -> {name: number of hops}. anchors: {sequence name: the 5-tuple PoseStream takes}.
    cfg.stream.fuse / fuse_weight as stream_eval: the fused columns, and a flush of its last window
    when a sequence ends (all hops of a push are fused by one launch; every anchor must then carry
    one ratio and one dataset). cfg.stream.carry and candidate_fn: as stream_eval (StreamPool
    carry=True; a sequence that takes over a stream starts with fresh ids). cfg.stream.warm, warm_mode and
    warm_iters: as stream_eval (StreamPool warm=True). cfg.stream.landmarks and lm_*: as stream_eval
    (StreamPool landmarks=True): a sequence that takes over a stream brings the intrinsics of its own box
    and starts with an empty map, and when it ends csv_dir/<name>_landmarks.csv takes its final snapshot.
    cfg.stream.motion and motion_*: as stream_eval (StreamPool motion=True): a sequence that takes over a stream
    starts with an empty history, and csv_dir/<name>_motion.csv takes one row per hop."""
    from .data import crop_resize_normalize
    from .stream import StreamPool, keypoint_query
    if not _get(cfg, "stream.enable", False):
        raise ValueError("stream_eval_pool is opt-in: set cfg.stream.enable")
    model.eval()
    window = int(_get(cfg, "stream.window", _get(cfg, "seqlen", 16)))
    size = int(_get(cfg, "train.img_size", 512))
    S = int(_get(cfg, "stream.streams", 4))
    query_fn = None
    carry = _stream_carry(cfg, sp, sift, candidate_fn, device)
    if query_points is None and not carry:
        sp = sp if sp is not None else _keypoint_init(cfg, device)
        query_fn = keypoint_query(sp, sift=sift, track_num=_get(cfg, "train.track_num", 512))
    mp = _get(cfg, "mixed_precision", "no")
    anchors = anchors or {}
    fuse, fuse_weight, default_anchor, fields = _stream_fuse(cfg, None)
    anchored = fuse or bool(anchors)
    if anchored and default_anchor is None:
        raise ValueError("stream_eval_pool: anchors without cfg.stream.fuse are not supported")
    lm = _stream_landmarks(cfg, fuse, carry)
    pnp = _stream_pnp(cfg, lm)
    motion = _stream_motion(cfg, fuse)
    if lm:  # (the uncropped intrinsics stand in until reset(sid, track_intr=...) brings each sequence's own)
        from .models.utils import INTRINSICS
        lm["track_intrs"] = [INTRINSICS[default_anchor[4]]] * S
    pool = StreamPool(model, streams=S, window=window, stride=int(_get(cfg, "stream.stride", 1)),
                      capacity=_get(cfg, "stream.capacity", None), query_fn=query_fn,
                      anchors=[default_anchor] * S if fuse else None,
                      precision=torch.bfloat16 if mp == "bf16" else torch.float32, fuse=fuse, fuse_weight=fuse_weight,
                      **carry, **lm, **pnp, **motion)
    if carry:
        fields = tuple(fields) + _carry_fields(carry)
    pnp_loggers = {}  # sequence name -> the logger of its <name>_pnp.csv
    motion_loggers = {}  # sequence name -> the logger of its <name>_motion.csv
    lasts = {}  # stream id -> (last result, its row): flushed when the sequence ends
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    seqs = iter(sequences)
    running = {}  # stream id -> (name, frame iterator, box, logger)
    hops = {}

    def next_frame(sid):
        """The next frame of stream sid's sequence, moving on to the next sequence when it ends."""
        while True:
            if sid not in running:
                nxt = next(seqs, None)
                if nxt is None:
                    return None
                name, frames_iter, box = nxt
                pool.reset(sid, anchor=anchors.get(name, default_anchor) if fuse else None,
                           track_intr=_track_intr(default_anchor[4], box, size) if lm else None)
                running[sid] = (name, iter(frames_iter), box, CsvLogger(os.path.join(csv_dir, f"{name}.csv"), fields))
                hops[name] = 0
                if pnp:
                    pnp_loggers[name] = CsvLogger(pnp_csv(running[sid][3].path), PNP_FIELDS)
                if motion:
                    motion_loggers[name] = CsvLogger(motion_csv(running[sid][3].path), MOTION_FIELDS)
            frame = next(running[sid][1], None)
            if frame is not None:
                return frame
            if fuse and sid in lasts:
                r, row = lasts.pop(sid)
                _log_hop(running[sid][3], fields, r, window, None, last=row)
            if lm:
                _log_landmarks(running[sid][3].path, pool.landmark_map, sid)
                if lm.get("lm_archive"):
                    _log_archive(running[sid][3].path, pool.landmark_map, sid)
            del running[sid]

    while True:
        new = [(sid, frame) for sid in range(S) for frame in [next_frame(sid)] if frame is not None]
        if not new:
            return hops
        ups = [torch.as_tensor(frame)[None].to(device) for _, frame in new]
        e0.record()
        frames = torch.cat([crop_resize_normalize(up, running[sid][2], (size, size)) for (sid, _), up in zip(new, ups)])
        results = pool.push(frames, streams=[sid for sid, _ in new], query_points=query_points)
        e1.record()
        for sid, r in results:
            e1.synchronize()
            name, logger = running[sid][0], running[sid][3]
            lasts[sid] = (r, _log_hop(logger, fields, r, window, e0.elapsed_time(e1)))
            if pnp:
                _log_pnp(pnp_loggers[name], hops[name], r, pool.landmark_map.stride)
            if motion:
                _log_motion(motion_loggers[name], hops[name], r)
            hops[name] += 1


# ------------------------------------------------------------------------------------------------
class CsvLogger:
    """abl_ours.py:9-22: header written once when the file is new, one DictWriter row per log()."""

    def __init__(self, path, fieldnames):
        import csv
        self.path, self.fieldnames, self._csv = path, list(fieldnames), csv
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        if not os.path.exists(path):
            with open(path, "w", newline="") as f:
                csv.DictWriter(f, fieldnames=self.fieldnames).writeheader()

    def log(self, row):
        with open(self.path, "a", newline="") as f:
            self._csv.DictWriter(f, fieldnames=self.fieldnames).writerow(row)


def test_fn(cfg, data_root=None, sp=None):
    """abl_ours.py:24-88, the evaluation entry point: accelerator with even_batches=False and the
    config's mixed precision, seed (+ rank), output_dir/test_results.csv (fields epoch, it, mode +
    TO_PLOT_METRICS), the eval loader with drop_last set on its batch sampler, the model from
    cfg.MODEL, build_optimizer over the eval loader (the scheduler supplies the logged lr),
    load_model_weights2 when train.resume_ckpt names a file, prepare, one eval pass of
    train_or_eval_fn at epoch -1, then the eval averages + lr as one CSV row on the main process.
    -> True. Differences: the model is always on the accelerator's device (the reference's
    device_placement=False leaves it where load_model_weights2 put it, on the device when a
    checkpoint is given), and `data_root` / cfg.data_root / $COMET_DATA_ROOT names the AMD
    dataset directory the reference hard-codes."""
    from .config import instantiate
    from .train import build_optimizer
    acc = CometAccelerator(mixed_precision=_get(cfg, "mixed_precision", "no"), even_batches=False)
    set_seed_and_print(int(_get(cfg, "seed", 0)))
    logger = None
    csv_path = os.path.join(_get(cfg, "output_dir", "."), "test_results.csv")
    if acc.is_main_process:
        logger = CsvLogger(csv_path, ["epoch", "it", "mode"] + list(TO_PLOT_METRICS))
        acc.print(f"Test results will be saved to {csv_path}")
    _, _, _, eval_dataloader = build_dataset(cfg, data_root, acc.device)
    inner = getattr(eval_dataloader, "loader", eval_dataloader)
    if getattr(inner, "batch_sampler", None) is not None:
        inner.batch_sampler.drop_last = True
    acc.print(f"Length of eval dataloader: {len(eval_dataloader)}")
    try:
        model = instantiate(cfg["MODEL"], _recursive_=False, cfg=cfg)
    except Exception as e:  # abl_ours.py:44-47
        raise RuntimeError(f"Failed to instantiate model: {e}")
    optimizer, lr_scheduler = build_optimizer(cfg, model, eval_dataloader)
    start_epoch = 0
    resume = _get(cfg, "train.resume_ckpt", "")
    if resume and os.path.isfile(resume):
        acc.print(f"Loading weights from specific file: {resume}")
        model = ckpt.load_model_weights2(model, resume, acc.device, _get(cfg, "relax_load", False))
    model, eval_dataloader, optimizer, lr_scheduler = acc.prepare(model, eval_dataloader, optimizer, lr_scheduler)
    acc.print(f"---------- Start Testing (Model Epoch: {start_epoch - 1}) ----------")
    stats = Stats(TO_PLOT_METRICS)
    lr = lr_scheduler.get_last_lr()[0]
    train_or_eval_fn(model, eval_dataloader, cfg, optimizer, stats, acc, lr_scheduler, training=False,
                     epoch=start_epoch - 1, sp=sp)
    stats.update({"lr": lr}, stat_set="eval")
    d = stats.get_epoch_averages()["eval"]
    if acc.is_main_process:
        row = {"epoch": d.get("epoch", start_epoch - 1), "it": d.get("it", 0), "mode": "eval"}
        row.update({k: d.get(k, "") for k in TO_PLOT_METRICS})
        logger.log(row)
        print(f"Test finished. Results saved to {csv_path}")
    return True
