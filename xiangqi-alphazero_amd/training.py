"""Train step and checkpoints -- the caller side of the self-play path.

`train_network` mirrors `AlphaZeroTrainer.train_network` (training/train.py:376-447): `num_epochs` passes over the whole
replay buffer in shuffled batches of `batch_size`, loss = -mean(sum(pi * log_softmax(logits))) + MSE(v, z), Adam,
gradient clipping at 1.0, one scheduler step per call, the same stats dict.  What differs is the data path: the
replay buffer holds the engine's compact 640-byte samples ON THE DEVICE (two logical samples per record: the position
and its mirror, in the reference's order s0, s0', s1, s1', ...), and every batch is materialised by one HIP kernel
(`xq_samples_to_batch`) instead of 70 KB/sample tuples going through a DataLoader.  The optimisation step itself is
torch autograd on the GPU (plumbing; <1 % of an iteration next to self-play).

`save_checkpoint` / `load_checkpoint` read and write the reference's files (train.py:537-579): `checkpoint_iter{N}.pt`
and `best_model.pt` with the same keys, so runs can move between the reference and this engine.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import hip, selfplay
from .sample_format import SAMPLE_DTYPE


@dataclass
class PositionGroups:
    """The records of a buffer grouped by position (`ReplayBuffer.position_groups`), on the device: group g holds the records
    members[offsets[g]:offsets[g + 1]] (ring indices, oldest first; member_mirrored says which of them enter mirrored), groups
    numbered by the age of their oldest member.  Valid for the buffer as it was when the groups were built."""
    offsets: torch.Tensor            # int32[n_groups + 1]
    members: torch.Tensor            # int32[n_records]
    member_mirrored: torch.Tensor    # uint8[n_records]
    n_groups: int
    sizes: torch.Tensor              # int64[n_groups]
    n_records: int


class ReplayBuffer:
    """FIFO of compact samples on the device; `max_size` counts LOGICAL samples like the reference's
    `deque(maxlen=max_buffer_size)` (train.py:206), i.e. max_size // 2 records."""

    def __init__(self, max_size: int = 50000, device="cuda", late_temperature: float = 0.3):
        self.device = torch.device(device)
        self.cap = max(1, max_size // 2)
        self.late_temperature = late_temperature
        self.store = torch.zeros((self.cap, hip.SAMPLE_BYTES), dtype=torch.uint8, device=self.device)
        self.count = 0          # records held
        self.head = 0           # next write position (ring)

    def __len__(self) -> int:
        return 2 * self.count

    def extend(self, samples) -> None:
        """Append finished samples, game order: a structured array of SAMPLE_DTYPE, or a uint8 tensor [n, 640] (device
        records of `SelfPlayEngine.drain_device` / `all_gather_records_device`: no host hop)."""
        if len(samples) == 0:
            return
        if isinstance(samples, torch.Tensor):
            raw = samples.view(-1, hip.SAMPLE_BYTES)
        else:
            raw = torch.from_numpy(np.ascontiguousarray(samples).view(np.uint8).reshape(len(samples), hip.SAMPLE_BYTES))
        raw = raw[-self.cap:].to(self.device)
        n = raw.shape[0]
        first = min(n, self.cap - self.head)
        self.store[self.head:self.head + first] = raw[:first]
        if n > first:
            self.store[:n - first] = raw[first:]
        self.head = (self.head + n) % self.cap
        self.count = min(self.cap, self.count + n)

    def extend_from_records(self, records, invalid: str = "raise", **selection) -> Dict[str, int]:
        """Append the samples of game records (`hip.records_to_samples`; `selection` = its movers, per_record_movers,
        skip_opening and skip_draws): one row per selected ply, a one-hot policy target at the move played and the game's
        result as the value target.  A record that does not convert (a malformed header, an illegal ply) raises XqError naming
        the record and the ply with invalid="raise"; with invalid="drop" it is left out whole, its rows masked out on the device
        before the extend.  -> {"games", "samples", "invalid"}: records read, rows appended, records that did not convert."""
        rows, info = rows_from_records(records, self.device, invalid, **selection)
        self.extend(rows)
        return info

    def _record_of(self, logical: torch.Tensor):
        """logical index (oldest first, s0, s0', s1, ...) -> (ring record index, flip flag)."""
        rec = torch.div(logical, 2, rounding_mode="floor")
        oldest = (self.head - self.count) % self.cap
        return ((rec + oldest) % self.cap).to(torch.int32), (logical % 2).to(torch.uint8)

    def root_stats_coverage(self) -> float:
        """The share of the held records that carry root statistics (has_root_stats, byte 116 of a record: an engine with
        root_stats=True wrote it); 0.0 for an empty buffer.  Counted on the device over the ring's live records."""
        if self.count == 0:
            return 0.0
        # a ring that has not wrapped holds its records at [0, count); a wrapped one is full
        mark = self.store[:self.count, 116] == 1
        return float(mark.sum().item()) / float(self.count)

    def policy_stats_coverage(self) -> float:
        """The share of the held records that carry policy statistics (has_policy_stats, byte 124 of a record:
        `selfplay.score_samples(write_back=True)` wrote it); 0.0 for an empty buffer."""
        if self.count == 0:
            return 0.0
        mark = self.store[:self.count, 124] == 1
        return float(mark.sum().item()) / float(self.count)

    def epoch_order(self, alpha: float, seed: int, epoch: int, generator=None, shuffle: bool = True) -> torch.Tensor:
        """The logical indices of one policy-surprise weighted epoch (int64, on the host): record r of the live records, oldest
        first, is drawn c_r times (xq_surprise_counts over the live records: uniform for alpha = 0, in proportion to the KL of the
        search target against the raw prior for alpha = 1), so logical samples 2r and 2r + 1 -- the position and its mirror --
        are each repeated c_r times; the list is then permuted by `torch.randperm(len, generator=generator)`."""
        if self.count == 0:
            return torch.zeros(0, dtype=torch.int64)
        # a ring that has not wrapped holds its records at [0, count); a wrapped one is full: the live records, in ring order
        counts = hip.surprise_counts(self.store[:self.count], alpha, seed, epoch)
        oldest = (self.head - self.count) % self.cap
        counts = torch.roll(counts, -oldest, 0).to("cpu", torch.int64)        # oldest first
        order = torch.repeat_interleave(torch.arange(2 * self.count), torch.repeat_interleave(counts, 2))
        return order[torch.randperm(order.numel(), generator=generator)] if shuffle else order

    def batch(self, logical: torch.Tensor, q_mix: float = 0.0):
        """-> states f32[B,15,10,9], pi f32[B,8100], z f32[B,1] for the given logical indices (device int64).  q_mix > 0: z is
        the q-mixed value target of xq_samples_to_batch_ex for the records that carry root statistics."""
        idx, flip = self._record_of(logical.to(self.device))
        b = idx.shape[0]
        states = torch.empty((b, 15, 10, 9), dtype=torch.float32, device=self.device)
        pi = torch.empty((b, hip.ACTION_SPACE), dtype=torch.float32, device=self.device)
        z = torch.empty((b, 1), dtype=torch.float32, device=self.device)
        opts = hip.BatchOpts(float(q_mix))
        hip.check(hip.lib().xq_samples_to_batch_ex(self.store.data_ptr(), idx.contiguous().data_ptr(),
                                                   flip.contiguous().data_ptr(), b, float(self.late_temperature),
                                                   C.byref(opts), states.data_ptr(), pi.data_ptr(), z.data_ptr(),
                                                   hip.stream_ptr(self.device)), "xq_samples_to_batch_ex")
        self._keep = (idx, flip)
        return states, pi, z


    def position_groups(self, mirror: bool = True) -> PositionGroups:
        """The live records grouped by position (board and side to move; with `mirror`, a position and its left-right mirror
        image are one group): keys by xq_position_keys over the records oldest first, a stable sort by key, the group heads by
        xq_position_group_heads (a full compare of side and canonical board: a key collision cannot merge two positions), a
        cumulative sum, and a relabelling by the oldest member.  sample_format.position_groups is the numpy reference."""
        n = self.count
        dev = self.device
        if n == 0:
            return PositionGroups(torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                                  torch.zeros(0, dtype=torch.uint8, device=dev), 0, torch.zeros(0, dtype=torch.int64, device=dev), 0)
        oldest = (self.head - self.count) % self.cap
        ring = ((torch.arange(n, device=dev) + oldest) % self.cap).to(torch.int32)      # row (age) -> ring index
        keys, mirrored = hip.position_keys(self.store, ring, mirror)
        order = torch.sort(keys, stable=True)[1]                 # any total order of the keys groups equal keys, in age order
        head = hip.position_group_heads(self.store, ring, order.to(torch.int32), keys, mirrored).to(torch.int64)
        gid_sorted = torch.cumsum(head, 0) - 1
        n_groups = int(gid_sorted[-1].item()) + 1
        first_row = order[head == 1]                             # the oldest member of each group: the sort is stable
        label = torch.empty(n_groups, dtype=torch.int64, device=dev)
        label[torch.sort(first_row, stable=True)[1]] = torch.arange(n_groups, device=dev)
        row_label = torch.empty(n, dtype=torch.int64, device=dev)
        row_label[order] = label[gid_sorted]
        rows = torch.sort(row_label, stable=True)[1]             # by group, age order inside a group
        sizes = torch.bincount(row_label, minlength=n_groups)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sizes, 0)]).to(torch.int32)
        return PositionGroups(offsets, ring[rows].contiguous(), mirrored[rows].contiguous(), n_groups, sizes, n)

    def batch_groups(self, groups: PositionGroups, logical: torch.Tensor, q_mix: float = 0.0):
        """-> states f32[B,15,10,9], pi f32[B,8100], z f32[B,1] of merged samples (xq_groups_to_batch): logical index 2 g + f is
        group g of `groups` under flip f; policy and value targets are the means over the group's records."""
        logical = logical.to(self.device)
        group = torch.div(logical, 2, rounding_mode="floor").to(torch.int32)
        flip = (logical % 2).to(torch.uint8)
        out = hip.groups_to_batch(self.store, groups.offsets, groups.members, groups.member_mirrored, group, flip,
                                  self.late_temperature, q_mix)
        self._keep = (group, flip)
        return out


def merge_duplicate_positions(config) -> bool:
    """`config.merge_duplicate_positions` (a reference TrainingConfig has no such key: off)."""
    return bool(getattr(config, "merge_duplicate_positions", False))


def merge_mirror_positions(config) -> bool:
    """`config.merge_mirror_positions` (absent: on): whether merging takes a position and its mirror image as one."""
    v = getattr(config, "merge_mirror_positions", True)
    return True if v is None else bool(v)


def prepare_ddp(model, device, group=None, native_bn: bool = False):
    """The data-parallel form of `model`, built ONCE and kept for the model's lifetime: BatchNorm -> SyncBatchNorm IN PLACE
    (same Parameters and buffers, same state_dict keys: checkpoints, `broadcast_weights` and the evaluators are unaffected)
    and one DistributedDataParallel wrapper (its construction broadcasts the parameters, so it is not repeated per call).
    SIDE EFFECT on the caller's model: from here on a training-mode forward is a collective -- every rank of `group` must
    take part in it; `train_network(ddp=False)` refuses such a model under a multi-rank group (`revert_sync_batchnorm`
    undoes the conversion).
    `native_bn` sets (or clears) on every converted layer the plain attribute `native_bn` (not a buffer, not in the state_dict): with
    it, the tower's and the stem's SyncBatchNorm run on the hand-written kernels when the model's `native_conv` is on
    (native_conv.sync_bn_act: the same group statistics, summed in float64); the heads' 32- and 4-channel layers stay with torch."""
    wrapper = model.__dict__.get("_xq_ddp")
    if wrapper is None:
        torch.nn.SyncBatchNorm.convert_sync_batchnorm(model, group)       # in place for the children
        device = torch.device(device)
        wrapper = torch.nn.parallel.DistributedDataParallel(
            model, device_ids=[device.index] if device.type == "cuda" else None, process_group=group, broadcast_buffers=False)
        model.__dict__["_xq_ddp"] = wrapper       # not a registered submodule (the wrapper already holds the model)
    for m in model.modules():
        if isinstance(m, torch.nn.SyncBatchNorm):
            m.native_bn = bool(native_bn)
    return wrapper


def revert_sync_batchnorm(model) -> None:
    """Undo `prepare_ddp`: every SyncBatchNorm becomes a BatchNorm2d again (same tensors) and the cached wrapper is dropped."""
    model.__dict__.pop("_xq_ddp", None)

    def walk(mod):
        for name, child in list(mod.named_children()):
            if isinstance(child, torch.nn.SyncBatchNorm):
                bn = torch.nn.BatchNorm2d(child.num_features, child.eps, child.momentum, child.affine, child.track_running_stats)
                bn.weight, bn.bias = child.weight, child.bias
                bn.running_mean, bn.running_var, bn.num_batches_tracked = child.running_mean, child.running_var, child.num_batches_tracked
                bn.train(child.training)
                setattr(mod, name, bn)
            else:
                walk(child)
    walk(model)


def train_network(model, optimizer, scheduler, buffer: ReplayBuffer, config, shuffle: bool = True,
                  generator: Optional[torch.Generator] = None, ddp: bool = False, group=None,
                  native_bn: bool = False, q_mix: Optional[float] = None,
                  surprise_weight: Optional[float] = None, merge_duplicates: Optional[bool] = None,
                  merge_mirror: Optional[bool] = None) -> Dict[str, float]:
    """One call of the reference's train_network (train.py:376-447) on the device-resident buffer.

    `ddp=True` under an initialised torch.distributed group (every rank holds the same buffer and the same weights, as
    AlphaZeroLoop keeps them): every batch is split across the ranks, BatchNorm statistics are synchronised (SyncBatchNorm:
    the batch statistics of the WHOLE batch, as on the reference's single device) and the gradients are summed by bucketed
    all-reduce overlapped with backward (DistributedDataParallel) -- the update is the reference's full-batch update, the
    replicas stay identical, and each GPU runs 1/world of the forward/backward work.  The conversion and the wrapper are
    made once per model (`prepare_ddp`, which documents the side effect on the caller's model).  The batch order comes
    from `generator` (or a generator seeded identically on every rank).  `native_bn=True` (ddp only; opt-in) runs the synchronised
    BatchNorm of the tower and the stem on the hand-written kernels instead of torch's SyncBatchNorm (`prepare_ddp`).

    `q_mix` (default: the config's `value_target_q_mix`, 0 when it has none): the value head regresses on
    (1 - q_mix) z + q_mix root_q for the samples that carry root statistics (`ReplayBuffer.batch`), on both paths.  With
    q_mix > 0 a buffer without a single such sample is refused: the option would silently do nothing.  With q_mix = 0 the
    step is unchanged; the stats gain "value_target_q_mix".

    `surprise_weight` (default: the config's `policy_surprise_weight`; None, absent and 0 mean off) = alpha in [0, 1]: every epoch
    draws record r c_r times instead of once (`ReplayBuffer.epoch_order`), the counts growing with the KL of the record's
    search target against the network's raw prior that `selfplay.score_samples` wrote into it (KataGo's policy-surprise
    weighting); an epoch then has about as many samples as before, in expectation.  The seed of the counts' rounding draws is
    one `torch.randint` draw from `generator` per call -- equal on every rank, so the data-parallel path needs nothing else.  With
    alpha > 0 a buffer without a single scored record is refused.  Off, the epoch loop is unchanged.  The stats gain
    "policy_surprise_weight", "policy_stats_coverage" (None when off: not measured) and "epoch_samples" (per epoch).

    `merge_duplicates` (default: the config's `merge_duplicate_positions`; absent means off): the records of one position -- and,
    unless `merge_mirror` (default: the config's `merge_mirror_positions`, absent: on) is False, of its mirror image -- are trained on as ONE sample per orientation whose
    policy and value targets are the means over those records (`ReplayBuffer.position_groups`, built once per call: the buffer
    does not change during a call, and every rank of a data-parallel step holds the same buffer, hence the same groups).  An epoch
    is then a permutation of 2 * n_groups logical samples (`ReplayBuffer.batch_groups`).  Together with policy_surprise_weight > 0
    it is refused.  The stats gain "merge_duplicate_positions", "distinct_positions", "merged_records" (records minus groups) and
    "largest_group" (False / None / None / None when off, and the epoch loop is unchanged)."""
    if len(buffer) < config.min_buffer_size:
        return {}
    if q_mix is None:                                  # self-play's reader of the key: None, the range, the Gumbel refusal
        q_mix = selfplay.root_stats_q_mix(config)
    q_mix = float(q_mix)
    if not 0.0 <= q_mix <= 1.0:
        raise hip.XqError(f"value_target_q_mix must be in [0, 1], got {q_mix}")
    if q_mix > 0.0 and buffer.root_stats_coverage() == 0.0:
        raise hip.XqError("value_target_q_mix > 0 but no sample in the replay buffer carries root statistics: "
                          "record them in self-play (record_root_stats / SelfPlayEngine(root_stats=True))")
    if surprise_weight is None:
        surprise_weight = selfplay.policy_surprise_weight(config)
    alpha = float(surprise_weight or 0.0)
    if not 0.0 <= alpha <= 1.0:
        raise hip.XqError(f"policy_surprise_weight must be in [0, 1], got {alpha}")
    if merge_duplicates is None:
        merge_duplicates = merge_duplicate_positions(config)
    merge = bool(merge_duplicates)
    if merge and alpha > 0.0:
        raise hip.XqError("merge_duplicate_positions and policy_surprise_weight > 0 cannot be combined: which of a merged group's "
                          "KLs should weight it is not defined")
    coverage = None
    if alpha > 0.0:
        coverage = buffer.policy_stats_coverage()
        if coverage == 0.0:
            raise hip.XqError("policy_surprise_weight > 0 but no sample in the replay buffer carries policy statistics: "
                              "score the samples in self-play (score_samples / selfplay.score_samples(write_back=True))")
    import torch.distributed as dist
    use_ddp = bool(ddp and dist.is_initialized())
    world = dist.get_world_size(group) if use_ddp else 1
    rank = dist.get_rank(group) if use_ddp else 0
    n = len(buffer)
    model.train()
    net = model
    if use_ddp:
        net = prepare_ddp(model, buffer.device, group, native_bn)
        if generator is None:                                              # one order for all ranks
            generator = torch.Generator().manual_seed(int(scheduler.last_epoch) * 7919 + 17)
    elif dist.is_initialized() and dist.get_world_size(group) > 1 and any(isinstance(m, torch.nn.SyncBatchNorm) for m in model.modules()):
        # a training-mode forward of this model is a collective; taken by a subset of the ranks it would hang
        raise hip.XqError("train_network(ddp=False): the model still carries SyncBatchNorm from a ddp step and the process "
                          "group has %d ranks; train with ddp=True on every rank or call revert_sync_batchnorm(model) first"
                          % dist.get_world_size(group))
    # the two losses of every batch are added up ON THE DEVICE in float64 (the same additions, in the same order, as the reference's
    # Python floats, train.py:421-423) and read once at the end: no host synchronisation inside the epoch loop
    totals = None                                                      # float64[2] on the losses' device
    batches = 0
    epoch_samples = []
    if alpha > 0.0:                                                    # one draw per call keys every epoch's rounding decisions
        surprise_seed = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator).item())
    groups = None
    if merge:                                                          # once per call: the buffer does not change during a call
        groups = buffer.position_groups(merge_mirror_positions(config) if merge_mirror is None else bool(merge_mirror))
        n = 2 * groups.n_groups
    for epoch in range(config.num_epochs):
        if alpha > 0.0:
            order = buffer.epoch_order(alpha, surprise_seed, epoch, generator, shuffle)
            n = order.numel()
        else:
            order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
        epoch_samples.append(int(n))
        for lo in range(0, n, config.batch_size):                     # drop_last=False
            idx = order[lo:lo + config.batch_size]
            full = idx.numel()
            scale = 1.0
            if use_ddp and full >= world:                              # this rank's slice of the batch
                idx = idx.tensor_split(world)[rank]
                scale = float(world)                                   # DDP averages the ranks' gradients
            if groups is not None:
                states, target_pi, target_z = buffer.batch_groups(groups, idx, q_mix)
            else:
                states, target_pi, target_z = buffer.batch(idx, q_mix)
            logits, value = net(states)
            if use_ddp and full >= world:
                # sums over the local slice, scaled so that DDP's average over ranks is the full-batch mean loss
                policy_loss = -torch.sum(target_pi * F.log_softmax(logits, dim=1)) / full
                value_loss = torch.sum((value - target_z) ** 2) / full
                loss = (policy_loss + value_loss) * scale
            else:                                                      # the reference's expressions (train.py:409-413)
                policy_loss = -torch.mean(torch.sum(target_pi * F.log_softmax(logits, dim=1), dim=1))
                value_loss = F.mse_loss(value, target_z)
                loss = policy_loss + value_loss
            optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            optimizer.step()
            pv = torch.stack([policy_loss.detach(), value_loss.detach()])
            if use_ddp and full >= world:
                dist.all_reduce(pv, group=group)                       # the slices' shares add up to the batch's losses
            totals = pv.double() if totals is None else totals + pv.double()
            batches += 1
    scheduler.step()
    total_p, total_v = totals.tolist() if totals is not None else (0.0, 0.0)
    return {"policy_loss": total_p / max(batches, 1), "value_loss": total_v / max(batches, 1),
            "total_loss": (total_p + total_v) / max(batches, 1), "learning_rate": optimizer.param_groups[0]["lr"],
            "value_target_q_mix": q_mix, "policy_surprise_weight": alpha, "policy_stats_coverage": coverage,
            "epoch_samples": epoch_samples, "merge_duplicate_positions": merge,
            "distinct_positions": groups.n_groups if merge else None,
            "merged_records": groups.n_records - groups.n_groups if merge else None,
            "largest_group": int(groups.sizes.max().item()) if merge else None}


def rows_from_records(records, device, invalid: str = "raise", **selection):
    """The sample rows of game records, on the device (`hip.records_to_samples`), with the records that do not convert (a
    malformed header, an illegal ply) either refused (invalid="raise": XqError naming the first such record and its ply) or left
    out whole (invalid="drop": their rows are masked out on the device) -> (rows uint8[m, 640], {"games", "samples", "invalid"})."""
    if invalid not in ("raise", "drop"):
        raise hip.XqError(f"invalid must be 'raise' or 'drop', got {invalid!r}")
    out = hip.records_to_samples(records, device=device, **selection)
    status, offsets, rows = out["status"], out["offsets"], out["samples"]
    bad = torch.nonzero(status != 0).reshape(-1)
    n_bad = int(bad.numel())
    if n_bad:
        if invalid == "raise":
            i = int(bad[0].item())
            st = int(status[i].item())
            what = f"ply {st - 1} is no legal move of its position" if st > 0 else "its header is malformed"
            raise hip.XqError(f"record {i} does not convert to samples: {what} ({n_bad} of {status.numel()} records do not; "
                              "invalid='drop' leaves them out)")
        counts = (offsets[1:] - offsets[:-1]).to(torch.int64)
        rows = rows[torch.repeat_interleave(status == 0, counts)]
    return rows, {"games": int(status.numel()), "samples": int(rows.shape[0]), "invalid": n_bad}


class _ConstantRate:
    """The scheduler of a supervised warm start: the learning rate stays what the optimizer holds, and the loop's own scheduler
    (whose lr_milestones count self-play iterations) is not stepped."""
    last_epoch = 0

    def step(self) -> None:
        pass


class _PretrainConfig:
    """The caller's config as `train_network` reads it for one supervised epoch: one epoch per call, no minimum buffer size,
    every other key the caller's."""

    def __init__(self, config):
        self._config = config
        self.num_epochs = 1
        self.min_buffer_size = 0

    def __getattr__(self, name):
        return getattr(self._config, name)


def pretrain_from_records(model, optimizer, records, config, epochs: int, invalid: str = "raise",
                          generator: Optional[torch.Generator] = None, merge_duplicates: Optional[bool] = None,
                          device=None, info: Optional[dict] = None, **selection) -> list:
    """A supervised warm start: `epochs` epochs of `train_network` over the samples of game records (`rows_from_records`;
    `selection` = hip.records_to_samples' movers, per_record_movers, skip_opening, skip_draws), in a fresh ReplayBuffer that
    holds every row (max_size = 2 x rows: the buffer counts logical samples, a position and its mirror).  The policy target of
    such a row is one-hot at the move played and the value target the game's result; `merge_duplicates` (default: the config's
    `merge_duplicate_positions`) averages the records of one position, which turns a teacher's tie-breaking draws into the
    distribution over its tied best moves.  q-mixing and policy-surprise weighting are off: the rows carry neither mark.  The
    learning rate is the optimizer's own throughout (a throwaway constant-rate scheduler).  -> one stats dict of
    `train_network` per epoch; `info`, when given, receives {"games", "samples", "invalid"}."""
    if isinstance(epochs, bool) or int(epochs) != epochs or int(epochs) < 1:
        raise hip.XqError(f"pretrain_from_records: epochs must be an integer >= 1, got {epochs!r}")
    if device is None:
        device = next(model.parameters()).device
    rows, counts = rows_from_records(records, device, invalid, **selection)
    if info is not None:
        info.update(counts)
    if rows.shape[0] == 0:
        raise hip.XqError("pretrain_from_records: the records select no sample")
    buffer = ReplayBuffer(2 * int(rows.shape[0]), device)       # late_temp is 0 in every row: the temperature is never read
    buffer.extend(rows)
    cfg, scheduler = _PretrainConfig(config), _ConstantRate()
    return [train_network(model, optimizer, scheduler, buffer, cfg, generator=generator, q_mix=0.0, surprise_weight=0.0,
                          merge_duplicates=merge_duplicates) for _ in range(int(epochs))]


def save_checkpoint(checkpoint_dir: str, iteration: int, current_model, best_model, optimizer, scheduler, total_games: int,
                    is_best: bool = False) -> str:
    """Writes the reference's two files with the reference's keys (train.py:537-567)."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    cfg = {"num_channels": current_model.num_channels, "num_res_blocks": current_model.num_res_blocks}
    path = os.path.join(checkpoint_dir, f"checkpoint_iter{iteration}.pt")
    torch.save({"iteration": iteration, "model_state_dict": current_model.state_dict(),
                "best_model_state_dict": best_model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                "scheduler_state_dict": scheduler.state_dict(), "config": cfg, "total_games": total_games}, path)
    if is_best:
        torch.save({"model_state_dict": best_model.state_dict(), "config": cfg, "iteration": iteration,
                    "total_games": total_games}, os.path.join(checkpoint_dir, "best_model.pt"))
    return path


def load_checkpoint(path: str, current_model, best_model, optimizer=None, scheduler=None, map_location="cpu") -> dict:
    """Reads a `checkpoint_iter*.pt` written by the reference or by save_checkpoint (train.py:569-579).
    `weights_only=True`: nothing in the file is executed."""
    ck = torch.load(path, map_location=map_location, weights_only=True)
    current_model.load_state_dict(ck["model_state_dict"])
    best_model.load_state_dict(ck["best_model_state_dict"])
    if optimizer is not None:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
    if scheduler is not None and "scheduler_state_dict" in ck:
        scheduler.load_state_dict(ck["scheduler_state_dict"])
    return {"iteration": ck["iteration"], "total_games": ck.get("total_games", 0), "config": ck.get("config", {})}
