"""Utterance-shard scatter / gather for multi-GPU restoration (one process per GPU).

Every utterance is restored independently (evaluation_proc/eval.py:119-134 iterates files;
eval-mode BatchNorm has no cross-sample coupling), so the path shards with no data-path
collective: rank r restores clips [lo_r, hi_r).  When the clips originate on one rank (the
reference's handler reads files on the host of a single process), rank 0 deals the shards out
and collects the results with grouped point-to-point sends: over xGMI rank 0 has a direct link
to each of its 7 peers, so a grouped isend/irecv drives all links concurrently (RCCL has no
native scatter).  Works with the `nccl` (= RCCL) backend on GPUs and `gloo` on CPU (tests).
"""
import time

import torch
import torch.distributed as dist

from . import clips as _clips


def world_rank():
    """(world, rank); a process that never initialised torch.distributed is a world of one."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def live_ranks(device):
    """Number of ranks that actually take part in collectives: an all-reduce of ones (1 without a process group)."""
    world, _ = world_rank()
    if world == 1:
        return 1
    t = torch.ones(1, device=device, dtype=torch.int32)
    dist.all_reduce(t)
    return int(t.item())


def shard_bounds(n, world):
    """Contiguous, balanced shards: [(lo, hi)] * world."""
    base, rem = divmod(n, world)
    out, lo = [], 0
    for r in range(world):
        hi = lo + base + (1 if r < rem else 0)
        out.append((lo, hi))
        lo = hi
    return out


def scatter_clips(full, n, length, device, src=0, dtype=torch.float32):
    """`full` (n, length) on rank `src` (ignored elsewhere) -> this rank's shard (n_r, length)."""
    world, rank = world_rank()
    bounds = shard_bounds(n, world)
    lo, hi = bounds[rank]
    if rank == src:
        ops = [dist.P2POp(dist.isend, full[a:b].contiguous(), r) for r, (a, b) in enumerate(bounds) if r != src and b > a]
        mine = full[lo:hi].clone()
    else:
        mine = torch.empty((hi - lo, length), device=device, dtype=dtype)
        ops = [dist.P2POp(dist.irecv, mine, src)] if hi > lo else []
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    return mine


def gather_clips(shard, n, length, device, dst=0):
    """Inverse of scatter_clips: returns (n, length) on rank `dst`, None elsewhere."""
    world, rank = world_rank()
    bounds = shard_bounds(n, world)
    if rank == dst:
        full = torch.empty((n, length), device=device, dtype=shard.dtype)
        lo, hi = bounds[rank]
        full[lo:hi] = shard
        ops = [dist.P2POp(dist.irecv, full[a:b], r) for r, (a, b) in enumerate(bounds) if r != dst and b > a]
    else:
        full = None
        ops = [dist.P2POp(dist.isend, shard.contiguous(), dst)] if shard.shape[0] > 0 else []
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    return full


def broadcast_state_dict(sd, device, src=0):
    """Weights for N ranks ("weights: one broadcast at start"): rank `src` holds `sd` (a
    state_dict of tensors, e.g. read from a checkpoint file once), every other rank passes None.  The key / shape / dtype
    table travels as one small object, all floating-point tensors as ONE flat fp32 buffer in ONE `dist.broadcast`
    (260 MB for the ResUNet, 150 MB for the vocoder: one ring over xGMI instead of 660 small ones); integer tensors
    (`num_batches_tracked`) are dropped -- the engines ignore them.  Returns a state_dict of CPU tensors on every rank
    (what `Engine.load_state_dict` takes).  A world of one returns `sd` unchanged."""
    world, rank = world_rank()
    if world == 1:
        return sd
    meta = [None]
    if rank == src:
        items = [(k, v) for k, v in sd.items() if isinstance(v, torch.Tensor) and v.is_floating_point()]
        meta[0] = [(k, tuple(v.shape)) for k, v in items]
    dist.broadcast_object_list(meta, src=src)
    table = meta[0]
    sizes = [int(torch.Size(shape).numel()) for _, shape in table]
    total = sum(sizes)
    if rank == src:
        flat = torch.cat([v.detach().reshape(-1).to(torch.float32) for _, v in items]) if total else torch.empty(0)
        flat = flat.to(device)
    else:
        flat = torch.empty(total, device=device, dtype=torch.float32)
    if total:
        dist.broadcast(flat, src=src)
    flat = flat.cpu()
    out, off = {}, 0
    for (k, shape), n in zip(table, sizes):
        out[k] = flat[off:off + n].reshape(shape)
        off += n
    return out


def checked_restore(engine, **kw):
    """engine_fn for restore_sharded / sharded_step / restore_sharded_lengths that keeps the 16-bit mode's guarantee on every
    rank: a batch whose vocoder activations left the fp16 range (VFX_FLAG_F16_SATURATED) is re-run on the split-bf16 twin, a
    negative mel (to_log's assert) raises (Engine.restore_gsr_checked; one device sync per call).  Called with `lengths` it
    restores a padded batch of clips of unequal length (Engine.restore_gsr_varlen_checked); `fn.bucket_key(L)` tells
    restore_sharded_lengths which clips may share such a call (all of them), `fn.bucket_len(L)` the row length to pad a batch
    whose longest clip has L samples to."""
    def fn(x, lengths=None):
        if lengths is None or len(set(int(v) for v in lengths)) == 1 and int(lengths[0]) == x.shape[-1]:
            return engine.restore_gsr_checked(x, **kw)
        return engine.restore_gsr_varlen_checked(x, lengths, **kw)
    # one bucket for everything (round 6: vfx_restore_gsr_varlen takes any mix of lengths -- the ResUNet per padded frame count inside
    # the call, the vocoder once over the batch); the clips of a call are neighbours in the length order, so little of a padded
    # batch is padding.  An engine that cannot run padded batches (Engine.supports_varlen: the 16-bit mode on the fp32 trunk)
    # buckets by exact length
    fn.bucket_key = (lambda L: 0) if engine.supports_varlen() else (lambda L: int(L))
    # a padded batch is handed over at the bucket's LARGEST length (padded_frames * hop - 1 samples: the same frame count), not at
    # the longest clip it happens to hold: the library caches a plan per (B, row length) (15 ms of host work to build, 0.6 ms to
    # reuse), and a real test set has a new longest length in nearly every bucket call
    if engine.supports_varlen():
        fn.bucket_len = lambda L: engine.padded_frames(L) * engine.hop - 1
    return fn


def restore_sharded(engine_fn, full, n, length, device, src=0):
    """scatter -> per-rank restore (engine_fn: (n_r, L) -> (n_r, L)) -> gather on `src`."""
    mine = scatter_clips(full, n, length, device, src)
    out = engine_fn(mine) if mine.shape[0] > 0 else mine
    return gather_clips(out, n, length, device, src)


def sharded_step(engine_fn, full, n, length, device, src=0, sync=None):
    """One step of the sharded job (BASELINE.json configs[3]) with its three phases clocked: returns
    (gathered (n, length) on `src` / None elsewhere, {"scatter_ms", "restore_ms", "gather_ms"}).
    `sync()` makes the device work of a phase finish before its clock is read (torch.cuda.synchronize on GPUs;
    nothing on CPU)."""
    sync = sync or (lambda: None)
    sync()
    t0 = time.perf_counter()
    mine = scatter_clips(full, n, length, device, src)
    sync()
    t1 = time.perf_counter()
    out = engine_fn(mine) if mine.shape[0] > 0 else mine
    sync()
    t2 = time.perf_counter()
    back = gather_clips(out, n, length, device, src)
    sync()
    t3 = time.perf_counter()
    return back, {"scatter_ms": (t1 - t0) * 1e3, "restore_ms": (t2 - t1) * 1e3, "gather_ms": (t3 - t2) * 1e3}


def deal_by_length(lengths, world):
    """"clip list sorted by length, dealt round-robin".  -> owner[i] = rank that restores clip i.
    Longest first: rank r never holds less audio than rank r + 1, and two ranks differ by at most the LONGEST clip (each
    round of the deal hands rank 0 a clip at least as long as everybody else's); ties keep the file order (the deal is a pure
    function of the lengths: every rank computes the same one)."""
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    owner = [0] * len(lengths)
    for pos, i in enumerate(order):
        owner[i] = pos % world
    return owner


def restore_sharded_lengths(engine_fn, clips, device, src=0, max_batch=128, dtype=torch.float32):
    """A test set of clips of ARBITRARY lengths (the reference iterates files of any length, one handler call each:
    evaluation_proc/eval.py:119-134) on N ranks.  `clips`: list of 1-D tensors on rank `src` (ignored elsewhere).  Returns the
    restored clips, same lengths, original order, on `src` (None elsewhere).

    * dealt by length (deal_by_length): the per-rank work is balanced without knowing the speed of anything;
    * every rank receives its clips as ONE flat buffer (one message per peer and direction, all of rank `src`'s links driven
      concurrently by the grouped isend / irecv) -- the lengths travel first, as one small object;
    * within a rank, clips that share `engine_fn.bucket_key(length)` run as one PADDED batch with their lengths
      (engine_fn(x (B, Lmax), lengths) -> (B, Lmax); `checked_restore`: ONE key for all clips since round 6 -- the call is
      vfx_restore_gsr_varlen, which runs the ResUNet per padded frame count and the vocoder per run of clips inside; the rows are
      padded to `engine_fn.bucket_len(longest)`) -- every clip's result is still the one its own batch-of-one call gives: the reflection
      at ITS end (fDomainHelper.py:26-28), the ResUNet's zero padding behind ITS last frame (unet.py:75-77), the vocoder stopped
      at ITS length (tests/test_gpu_surface.py).  An engine_fn without `bucket_key` gets clips of EQUAL length only
      ((B, L) -> (B, L), rounds 1-4).  At most `max_batch` clips per call;
    * an exception on one rank (to_log's assert, a twin that cannot be created) is raised on EVERY rank after the restore phase
      instead of leaving the others waiting in the gather;
    * a world of one is the length-bucketing helper for a single GPU (no process group needed)."""
    world, rank = world_rank()
    meta = [None]
    if rank == src:
        meta[0] = [int(c.shape[-1]) for c in clips]
    if world > 1:
        dist.broadcast_object_list(meta, src=src)
    lengths = meta[0]
    owner = deal_by_length(lengths, world)
    mine = [i for i in range(len(lengths)) if owner[i] == rank]
    total = sum(lengths[i] for i in mine)
    # ---- scatter: one flat buffer per rank
    if rank == src:
        ops, flat = [], None
        for r in range(world):
            idx = [i for i in range(len(lengths)) if owner[i] == r]
            if not idx:
                continue
            buf = torch.cat([clips[i].reshape(-1).to(device=device, dtype=dtype) for i in idx])
            if r == src:
                flat = buf
            else:
                ops.append(dist.P2POp(dist.isend, buf, r))
        if flat is None:
            flat = torch.empty(0, device=device, dtype=dtype)
    else:
        flat = torch.empty(total, device=device, dtype=dtype)
        ops = [dist.P2POp(dist.irecv, flat, src)] if total else []
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    # ---- restore: one padded batch per bucket (equal lengths when the engine function cannot take a length vector)
    pieces, off = {}, 0
    for i in mine:
        pieces[i] = flat[off:off + lengths[i]]
        off += lengths[i]
    key_of = getattr(engine_fn, "bucket_key", None)
    buckets = {}
    for i in mine:
        buckets.setdefault(key_of(lengths[i]) if key_of else lengths[i], []).append(i)
    done, failure = {}, None
    try:
        for k in sorted(buckets, reverse=True):
            idx = sorted(buckets[k], key=lambda i: (-lengths[i], i))
            for a in range(0, len(idx), max_batch):
                chunk = idx[a:a + max_batch]
                lens = [lengths[i] for i in chunk]
                if min(lens) == max(lens):
                    out = engine_fn(torch.stack([pieces[i] for i in chunk]))
                else:
                    blen = getattr(engine_fn, "bucket_len", None)
                    x = _clips.pad([pieces[i] for i in chunk], device, dtype, width=blen(max(lens)) if blen else None)
                    out = engine_fn(x, lens)
                for j, i in enumerate(chunk):
                    done[i] = out[j, :lengths[i]]
    except Exception as e:       # raised below, on every rank: nobody may be left waiting in the gather
        failure = e
    if world > 1:
        bad = torch.tensor([1 if failure is not None else 0], device=device, dtype=torch.int32)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if int(bad.item()) and failure is None:
            raise RuntimeError("restore_sharded_lengths: the restore failed on another rank")
    if failure is not None:
        raise failure
    back = torch.cat([done[i].reshape(-1) for i in mine]) if mine else torch.empty(0, device=device, dtype=dtype)
    # ---- gather
    if rank == src:
        bufs, ops = {src: back}, []
        for r in range(world):
            n_r = sum(lengths[i] for i in range(len(lengths)) if owner[i] == r)
            if r != src and n_r:
                bufs[r] = torch.empty(n_r, device=device, dtype=back.dtype)
                ops.append(dist.P2POp(dist.irecv, bufs[r], r))
    else:
        ops = [dist.P2POp(dist.isend, back.contiguous(), src)] if total else []
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    if rank != src:
        return None
    result, offs = [None] * len(lengths), {r: 0 for r in range(world)}
    for i in range(len(lengths)):
        r = owner[i]
        result[i] = bufs[r][offs[r]:offs[r] + lengths[i]]
        offs[r] += lengths[i]
    return result


def selfcheck(device, n=11, length=4096):
    """Round-trip a small tensor through scatter/gather; raises on mismatch."""
    _, rank = world_rank()
    full = torch.arange(n * length, device=device, dtype=torch.float32).reshape(n, length) if rank == 0 else None
    back = restore_sharded(lambda x: x * 2.0, full, n, length, device)
    if rank == 0 and not torch.equal(back, full * 2.0):
        raise RuntimeError("scatter/gather round trip mismatch")
    return True
