"""Multi-GPU sharding of independent instances (one process per GPU).

Instances are independent simulations, so the path shards with no data-path
collective: rank r owns instances [r * per_rank, (r + 1) * per_rank) and seeds them
base + global index (the reference seeds one run with rand.Seed(seed + 1),
snapshot_test.go:20).  After the timed region the ranks all-reduce a handful of int64
checksums and take the max of their elapsed times -- RCCL over xGMI when the tensors
live on the GPU (backend "nccl"), gloo on CPU in tests.
"""
import numpy as np
import torch
import torch.distributed as dist


def shard(per_rank, rank, seed_base):
    """(first global instance, seed of that instance) for this rank."""
    first = rank * per_rank
    return first, seed_base + first


def reduce_results(elapsed_s, sums, device):
    """Max elapsed time and summed int64 checksums over all ranks."""
    t = torch.tensor([float(elapsed_s)], dtype=torch.float64, device=device)
    s = torch.tensor([int(v) for v in sums], dtype=torch.int64, device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(s, op=dist.ReduceOp.SUM)
    return float(t.item()), [int(v) for v in s.tolist()]


def reduce_max(values, device):
    """Elementwise max of float values over all ranks."""
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return [float(v) for v in t.tolist()]


def reduce_stats(stats, device):
    """A rank's SnapshotStats (ChandyLamportSim.snapshot_stats of its shard) reduced over all
    ranks: one all_reduce each -- SUM, MIN, MAX -- over the three sections of the flat array
    (the int64 sums wrap modulo 2**64, like the sums of squares themselves).  Every rank must
    pass the same layout.  Returns a new SnapshotStats; without an initialised group, a copy."""
    L = stats.layout
    t = torch.from_numpy(stats.raw.copy()).to(device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for lo, hi, op in ((L["sum_begin"], L["sum_end"], dist.ReduceOp.SUM),
                           (L["min_begin"], L["min_end"], dist.ReduceOp.MIN),
                           (L["max_begin"], L["max_end"], dist.ReduceOp.MAX)):
            part = t[lo:hi].contiguous()
            dist.all_reduce(part, op=op)
            t[lo:hi] = part
    return type(stats)(L, t.cpu().numpy())


def reduce_crosstab(xt, device):
    """A rank's SnapshotCrosstab (ChandyLamportSim.snapshot_crosstab of its shard) reduced over all
    ranks, as reduce_stats: SUM over the counters, sums and cells (wrapping modulo 2**64), MIN and
    MAX over the extrema.  Every rank must pass the same axes.  Returns a new SnapshotCrosstab;
    without an initialised group, a copy."""
    t = torch.from_numpy(xt.raw.copy()).to(device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for lo, hi, op in ((0, 8, dist.ReduceOp.SUM), (8, 10, dist.ReduceOp.MIN), (10, 12, dist.ReduceOp.MAX),
                           (12, t.numel(), dist.ReduceOp.SUM)):
            part = t[lo:hi].contiguous()
            dist.all_reduce(part, op=op)
            t[lo:hi] = part
    return type(xt)(tuple(a.copy() for a in xt.axes), t.cpu().numpy())


def gather_census(census, first_instance, device):
    """A rank's SnapshotCensus (ChandyLamportSim.snapshot_census of its shard, whose instance 0 is
    global instance `first_instance`) combined over all ranks: one all_gather of the (class
    count, first instance) pairs sizes one all_gather of the class rows padded to the longest,
    and the parts merge with each rank's first instance as offset (SnapshotCensus.merge; a
    truncated census raises ValueError there).  Returns a new SnapshotCensus, the same on every
    rank, with global instance indices; without an initialised group, a copy."""
    cls = type(census)
    mine = cls(census.snapshot_id, census.instances, census.ok, census.sample, census.n_classes, census.classes.copy())
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return mine
    head = allgather_ints([mine.n_returned, first_instance, mine.instances, mine.ok, mine.sample, mine.n_classes],
                          device)
    words = mine.classes.dtype.itemsize // 8
    rows = np.zeros((max(int(head[:, 0].max()), 1), words), dtype=np.int64)
    rows[:mine.n_returned] = mine.classes.view(np.int64).reshape(-1, words)
    t = torch.from_numpy(rows).to(device)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    out = None
    for r, part in enumerate(parts):
        k, first, instances, ok, sample, n_classes = (int(v) for v in head[r])
        classes = part.cpu().numpy()[:k].reshape(-1).view(mine.classes.dtype)
        c = cls(mine.snapshot_id, instances, ok, sample, n_classes, classes)
        empty = cls(mine.snapshot_id, 0, 0, 0, 0, classes[:0])
        out = empty.merge(c, offset=first) if out is None else out.merge(c, offset=first)
    return out


def gather_groups(groups, first_instance, device):
    """A rank's SnapshotGroups (ChandyLamportSim.snapshot_groups of its shard, whose instance 0 is
    global instance `first_instance`) combined over all ranks, in the manner of gather_census: one
    all_gather of the heads sizes one all_gather of the rows -- the class words plus the values --
    padded to the longest, and the parts merge with each rank's first instance as offset
    (SnapshotGroups.merge; truncated groups raise ValueError there).  Every rank passes the same
    terms.  Returns a new SnapshotGroups, the same on every rank, with global instance indices;
    without an initialised group, a copy."""
    cls = type(groups)
    mine = cls(groups.terms.copy(), groups.instances, groups.ok, groups.sample, groups.n_groups, groups.groups.copy(),
               groups.values.copy())
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return mine
    head = allgather_ints([mine.n_returned, first_instance, mine.instances, mine.ok, mine.sample, mine.n_groups],
                          device)
    words, n_terms = mine.groups.dtype.itemsize // 8, mine.terms.size
    rows = np.zeros((max(int(head[:, 0].max()), 1), words + n_terms), dtype=np.int64)
    rows[:mine.n_returned, :words] = mine.groups.view(np.int64).reshape(-1, words)
    rows[:mine.n_returned, words:] = mine.values
    t = torch.from_numpy(rows).to(device)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    out = cls(mine.terms.copy(), 0, 0, 0, 0, mine.groups[:0], mine.values[:0])
    for r, part in enumerate(parts):
        k, first, instances, ok, sample, n_groups = (int(v) for v in head[r])
        part = part.cpu().numpy()[:k]
        rows_g = np.ascontiguousarray(part[:, :words]).reshape(-1).view(mine.groups.dtype)
        out = out.merge(cls(mine.terms.copy(), instances, ok, sample, n_groups, rows_g, part[:, words:]), offset=first)
    return out


def gather_selection(sel, first_instance, device):
    """A rank's SnapshotSelection (ChandyLamportSim.select_instances of its shard, whose instance 0
    is global instance `first_instance`) combined over all ranks, in the manner of gather_census:
    one all_gather of the heads sizes one all_gather of the (instance, tick) rows padded to the
    longest, and the parts merge with each rank's first instance as offset
    (SnapshotSelection.merge; a truncated selection raises ValueError there).  Returns a new
    SnapshotSelection, the same on every rank, with global instance indices; without an
    initialised group, a copy."""
    cls = type(sel)
    mine = cls(sel.snapshot_id, sel.instances, sel.ok, sel.sample, sel.n_match, sel.insts.copy(),
               None if sel.ticks is None else sel.ticks.copy())
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return mine
    head = allgather_ints([mine.n_returned, first_instance, mine.instances, mine.ok, mine.sample, mine.n_match,
                           mine.ticks is not None], device)
    rows = np.zeros((max(int(head[:, 0].max()), 1), 2), dtype=np.int64)
    rows[:mine.n_returned, 0] = mine.insts
    if mine.ticks is not None:
        rows[:mine.n_returned, 1] = mine.ticks
    t = torch.from_numpy(rows).to(device)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    out = None
    for r, part in enumerate(parts):
        k, first, instances, ok, sample, n_match, has_ticks = (int(v) for v in head[r])
        got = part.cpu().numpy()[:k]
        c = cls(mine.snapshot_id, instances, ok, sample, n_match, got[:, 0], got[:, 1] if has_ticks else None)
        empty = cls(mine.snapshot_id, 0, 0, 0, 0, got[:0, 0], got[:0, 1] if has_ticks else None)
        out = empty.merge(c, offset=first) if out is None else out.merge(c, offset=first)
    return out


def gather_topk(top, first_instance, device):
    """A rank's SnapshotTopK (ChandyLamportSim.snapshot_topk of its shard, whose instance 0 is
    global instance `first_instance`) combined over all ranks, in the manner of gather_selection:
    one all_gather of the heads sizes one all_gather of the (instance, value) rows padded to the
    longest, and the parts merge with each rank's first instance as offset (SnapshotTopK.merge,
    which is exact: the top-k of a union lies within the union of the parts' top-k).  Every rank
    passes the same term, direction and k.  Returns a new SnapshotTopK, the same on every rank,
    with global instance indices; without an initialised group, a copy."""
    cls = type(top)
    mine = cls(top.term.copy(), top.descending, top.k, top.instances, top.ok, top.sample, top.insts.copy(),
               top.values.copy())
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return mine
    head = allgather_ints([mine.n_returned, first_instance, mine.instances, mine.ok, mine.sample], device)
    rows = np.zeros((max(int(head[:, 0].max()), 1), 2), dtype=np.int64)
    rows[:mine.n_returned, 0] = mine.insts
    rows[:mine.n_returned, 1] = mine.values
    t = torch.from_numpy(rows).to(device)
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t)
    out = cls(mine.term.copy(), mine.descending, mine.k, 0, 0, 0, rows[:0, 0], rows[:0, 1])
    for r, part in enumerate(parts):
        k, first, instances, ok, sample = (int(v) for v in head[r])
        got = part.cpu().numpy()[:k]
        out = out.merge(cls(mine.term.copy(), mine.descending, mine.k, instances, ok, sample, got[:, 0], got[:, 1]),
                        offset=first)
    return out


# ---- exchange layer of the graph-partitioned mode ---------------------
# One simulation whose nodes are split into rank ranges exchanges, every tick, records
# addressed to the owners of other nodes (deliveries, broadcast-trigger reports, draw
# bases).  Records are fixed-width int64 rows; one all-to-all of counts sizes one
# all-to-all of the rows (RCCL over xGMI for device tensors, gloo for host tensors).

def exchange_rows(rows_by_dest, width, device="cpu"):
    """rows_by_dest[r]: int64 array [k_r, width] for rank r.  Returns the list of the
    arrays every rank addressed to this one, in source-rank order."""
    world = dist.get_world_size()
    counts = torch.tensor([len(r) for r in rows_by_dest], dtype=torch.int64, device=device)
    recv_counts = torch.empty_like(counts)
    dist.all_to_all_single(recv_counts, counts)
    send = torch.cat([torch.as_tensor(r, dtype=torch.int64).reshape(-1, width) for r in rows_by_dest]).to(device) \
        if any(len(r) for r in rows_by_dest) else torch.zeros((0, width), dtype=torch.int64, device=device)
    rc = recv_counts.tolist()
    recv = torch.empty((sum(rc), width), dtype=torch.int64, device=device)
    dist.all_to_all_single(recv.view(-1), send.reshape(-1).contiguous(),
                           output_split_sizes=[c * width for c in rc],
                           input_split_sizes=[len(r) * width for r in rows_by_dest])
    out, o = [], 0
    host = recv.cpu().numpy()
    for c in rc:
        out.append(host[o:o + c])
        o += c
    return out


def allgather_ints(values, device="cpu"):
    """[world, len(values)] int64: every rank's values."""
    t = torch.tensor([int(v) for v in values], dtype=torch.int64, device=device)
    out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return torch.stack(out).cpu().numpy()
