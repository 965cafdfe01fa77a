"""Monte-Carlo DoA sweep (restatement of paper_plots/target_snn_localization.py:435-467 as a batched,
shardable harness).  The script's loop carries no state between trials except the RNG stream, so trials
shard contiguously across ranks (one process per GPU); the only exchange is one small all-gather of
per-trial results at the end (RCCL over xGMI when the process group is "nccl").

parity mode      every rank replays the reference's global NumPy stream (rand(1) then randn(T, M) per trial,
                 legacy MT19937) and keeps its own shard, so results are identical to the single-process
                 reference for any world size.
throughput mode  DoAs from a seeded host generator, clean array signals synthesised on the device
                 (csrc/synth.hip, bit-exact with np.interp), noise from the Philox-4x32-10 + Box-Muller kernel
                 (csrc/rng.hip), numbered by global trial so that the draw does not depend on the sharding.

Sweeps: noisy_target_sweep (target_snn_localization.py:435-467), speech_target_sweep (:213-245), xylo_target_sweep
(target_xylo_localization.py:540-608; integer-LIF stage parity-unpinned), music_noisy_sweep / music_speech_sweep (the MUSIC twins,
target_localization_MUSIC.py), multi_target_sweep (K simultaneous targets, the statistical counterpart of
paper_plots/multiple_targets_*.py: K peaks per trial, matched errors and resolution rate), windowed_target_sweep (the noisy-target
sweep with the time-resolved read-out: one estimate per window of every trial), moving_target_sweep (a moving target scored per
frame, target_snn_localization.py:585-628), xylo_moving_target_sweep (the same read from the Xylo network's spikes,
target_xylo_localization.py:672-789; integer-LIF stage parity-unpinned).

Every sweep runs through ONE trial loop, `_monte_carlo`: shard range, ShardStore and resume, the parity replay of the global stream
(also across skipped trials), the throughput range loop, the flush of a finished batch, the one all-gather.  A sweep hands it only
what is its own: how a trial's truth is drawn, a host trial (parity) and a device batch (throughput), the per-trial result fields,
the read-out that fills them and its store key entries; it builds its result dict from what the loop returns.
"""
import os
import zlib

import numpy as np

from .snn_beamformer import synthesize_array_signal


def shard_range(total, rank, world_size):
    """Contiguous shard [lo, hi) of `total` trials for `rank`; sizes differ by at most one."""
    base, rem = divmod(total, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def doa_error(doa_est, doa_true):
    """arcsin|sin(est - true)| (target_snn_localization.py:466; pi-periodic by construction)."""
    return np.arcsin(np.abs(np.sin(doa_est - doa_true)))


class ShardStore:
    """Per-shard result persistence of a sweep (`out_dir=`): every finished device batch of a rank is written as ONE small `.npy`
    (a structured array {trial i8, doa f8, index i8, pmax f8}, 32 bytes per trial, written to a temporary name and renamed: a file
    either exists completely or not at all), under a directory keyed by everything the results depend on -- sweep, seed, mode, the
    SNR of every trial, the DoA grid, the hash of bf_mat and of the test signal -- so a rerun with the same arguments finds its own
    results and any change of them starts a fresh directory.  A rerun loads what exists and computes only the trials that are
    missing; in parity mode the reference's MT19937 stream is still replayed for the skipped trials, so the results are identical to an
    uninterrupted run -- also when the world size changed in between (coverage is per trial, not per shard).
    `rec`: the record dtype of a sweep whose trials hold more than that (K or nW columns, a further field); it starts with `trial`.
    The reference keeps its sweeps' results the same way, at the end of the script (ref:paper_plots/snn_localization_benchmark.py:588-592,
    ref:paper_plots/target_snn_localization.py:525); a 16 384-trial sweep over 8 ranks should not restart from zero."""

    REC = np.dtype([("trial", "<i8"), ("doa", "<f8"), ("index", "<i8"), ("pmax", "<f8")])

    def __init__(self, out_dir, sweep, total, *, rec=None, **key):
        import hashlib
        import json

        def h(v):
            if isinstance(v, np.ndarray):
                a = np.ascontiguousarray(v)
                return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape), "dtype": str(a.dtype)}
            if isinstance(v, (np.integer, np.floating)):
                return v.item()
            return v

        self.meta = {"sweep": sweep, "total": int(total), "format": 1, **{k: h(v) for k, v in sorted(key.items())}}
        blob = json.dumps(self.meta, sort_keys=True).encode()
        self.key = hashlib.sha256(blob).hexdigest()[:16]
        self.dir = os.path.join(str(out_dir), f"{sweep}-{self.key}")
        os.makedirs(self.dir, exist_ok=True)
        meta_path = os.path.join(self.dir, "meta.json")
        if not os.path.exists(meta_path):
            tmp = f"{meta_path}.tmp-{os.getpid()}"
            with open(tmp, "wb") as f:
                f.write(blob)
            os.replace(tmp, meta_path)  # (several ranks may race: they all write the same bytes)
        self.total = int(total)
        self.REC = self.REC if rec is None else np.dtype(rec)
        self.have = np.zeros(self.total, dtype=bool)
        self.rec = np.zeros(self.total, dtype=self.REC)
        self.files_loaded = 0
        self.trials_loaded = 0
        self.files_written = 0
        for name in sorted(os.listdir(self.dir)):
            if not (name.startswith("trials_") and name.endswith(".npy")):
                continue
            try:
                a = np.load(os.path.join(self.dir, name))
            except (OSError, ValueError):
                continue  # (cannot happen with the rename protocol; a damaged file is simply recomputed)
            if a.dtype != self.REC or a.ndim != 1 or len(a) == 0 or a["trial"].min() < 0 or a["trial"].max() >= self.total:
                continue
            self.rec[a["trial"]] = a
            self.have[a["trial"]] = True
            self.files_loaded += 1
        self.trials_loaded = int(self.have.sum())

    def covered(self, lo, hi):
        return bool(self.have[lo:hi].all())

    def put(self, trials, doa, index=0, pmax=0.0, **extra):
        """Persist one finished batch (any set of trial numbers) and mark it done (`extra`: further fields of the record dtype)."""
        trials = np.asarray(trials, dtype=np.int64)
        if len(trials) == 0:
            return
        a = np.zeros(len(trials), dtype=self.REC)
        a["trial"], a["doa"], a["index"], a["pmax"] = trials, doa, index, pmax
        for k, v in extra.items():
            a[k] = v
        # (the name carries a checksum of the trial numbers: two different sets with the same bounds and size -- resumed runs under
        #  different world sizes -- never overwrite each other's records)
        name = f"trials_{int(trials.min()):08d}_{int(trials.max()) + 1:08d}_{len(trials)}_{zlib.crc32(np.ascontiguousarray(trials).tobytes()):08x}.npy"
        tmp = os.path.join(self.dir, f".tmp-{os.getpid()}-{name}")
        with open(tmp, "wb") as f:
            np.save(f, a)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, os.path.join(self.dir, name))
        self.rec[trials] = a
        self.have[trials] = True
        self.files_written += 1

    def stats(self):
        return {"dir": self.dir, "files_loaded": self.files_loaded, "trials_loaded": self.trials_loaded, "files_written": self.files_written}


def gather_shards(local, total, rank, world_size, group=None, bounds=None, stats=None):
    """The sweep's one exchange step: all-gather the per-trial result arrays of contiguous shards; returns the
    full-length arrays on every rank.  `local` is a dict name -> numpy array, 1-d or [n, W] with one row per item (this rank's shard; any
    mix of dtypes and widths).
    ONE collective whatever the number of arrays: every rank packs its arrays into a struct-of-arrays byte record (each array
    padded to the widest shard and to 8 bytes), one `all_gather_into_tensor` moves the records (RCCL over xGMI when the group is
    "nccl": one host -> device copy, one collective, one device -> host copy), every rank unpacks.  `bounds(r) -> (lo, hi)`
    overrides the default `shard_range(total, r, world_size)` partition.  `stats` (a dict, optional) receives `exchange_ms` (wall
    time of pack + collective + unpack), `bytes_per_rank` and `collectives`."""
    import time

    if bounds is None:
        bounds = lambda r: shard_range(total, r, world_size)  # noqa: E731
    if world_size == 1:
        if stats is not None:
            stats.update(exchange_ms=0.0, bytes_per_rank=0, collectives=0)
        return {k: np.asarray(v) for k, v in local.items()}
    import torch
    import torch.distributed as dist

    t0 = time.perf_counter()
    backend = dist.get_backend(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    spans = [bounds(r) for r in range(world_size)]
    width = max(hi - lo for lo, hi in spans)  # padded shard length (items)
    keys = list(local)
    arrs = {k: np.ascontiguousarray(local[k]) for k in keys}
    n_local = spans[rank][1] - spans[rank][0]
    for k in keys:
        if arrs[k].ndim not in (1, 2) or len(arrs[k]) != n_local:
            raise ValueError(f"gather_shards: '{k}' has shape {arrs[k].shape}, this rank's shard holds {n_local} items")
    # record layout: the arrays one behind the other, each `width` items (rows) of its dtype, 8-byte aligned
    item = {k: arrs[k].dtype.itemsize * int(np.prod(arrs[k].shape[1:])) for k in keys}  # bytes per item
    offs, off = {}, 0
    for k in keys:
        offs[k] = off
        off += (width * item[k] + 7) & ~7
    rec = np.zeros(max(off, 8), dtype=np.uint8)
    for k in keys:
        v = arrs[k]
        rec[offs[k] : offs[k] + v.nbytes] = v.reshape(-1).view(np.uint8)
    buf = torch.from_numpy(rec).to(dev)
    full = torch.empty(len(rec) * world_size, dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(full, buf, group=group)
    full = full.cpu().numpy().reshape(world_size, len(rec))
    out = {}
    for k in keys:
        parts = [full[r, offs[k] : offs[k] + (hi - lo) * item[k]].view(arrs[k].dtype) for r, (lo, hi) in enumerate(spans)]
        out[k] = np.concatenate(parts).reshape((-1,) + arrs[k].shape[1:])
    if stats is not None:
        stats.update(exchange_ms=(time.perf_counter() - t0) * 1e3, bytes_per_rank=int(len(rec)), collectives=1)
    return out


def sharded_design(design_fn, doa_list, rank=0, world_size=1, group=None):
    """`design_from_template` sharded over the DoA grid (the G columns of bf_mat are independent units):
    every rank designs the columns of its contiguous DoA shard with `design_fn(doa_sublist) -> [2M, n_local]` and one
    all-gather assembles the full [2M, G] matrix on every rank (RCCL when the group is "nccl")."""
    doa_list = np.asarray(doa_list, dtype=np.float64)
    G = len(doa_list)
    lo, hi = shard_range(G, rank, world_size)
    local = np.asarray(design_fn(doa_list[lo:hi]), dtype=np.float64)
    if local.ndim != 2 or local.shape[1] != hi - lo:
        raise ValueError(f"design_fn returned shape {local.shape} for {hi - lo} DoAs")
    rows = local.shape[0]
    if world_size == 1:
        return local
    # one gather of `rows` doubles per DoA: flatten column-major so that a shard is a contiguous run of items
    flat = gather_shards({"cols": np.ascontiguousarray(local.T).ravel()}, G * rows, rank, world_size, group=group,
                         bounds=lambda r: tuple(rows * v for v in shard_range(G, r, world_size)))
    return flat["cols"].reshape(G, rows).T.copy()


def _in_batches(sig_batch, max_batch, one):
    """`one(slice)` -> a tuple of per-trial results (arrays, or device tensors) for every slice of at most `max_batch` trials of
    `sig_batch`; returns the tuple of their concatenations."""
    parts = [one(sig_batch[s : s + max_batch]) for s in range(0, len(sig_batch), max_batch)]

    def cat(col):
        if isinstance(col[0], np.ndarray):
            return np.concatenate(col)
        import torch

        return torch.cat(col)

    return tuple(cat(col) for col in zip(*parts))


def _argmax_and_power(out):
    a = out["argmax"].cpu().numpy().astype(np.int64)
    return a, out["power"].cpu().numpy()[np.arange(len(a)), a]


def _peaks_and_power(out):
    return out["peaks"].cpu().numpy().astype(np.int64), out["peak_power"].cpu().numpy()


def device_localizer(beamf, bf_mat, max_batch=1100, num_sources=None, doa_list=None, min_separation=None, rel_threshold=0.0, window=None,
                     hop=None):
    """Default localizer: the HIP pipeline (power + arg-max, no T x G temporary).  With num_sources=K (and doa_list) it returns the
    multi-source read-out instead: (peaks [B, K] int64, peak_power [B, K]) (multi_target_sweep); with window=N (and hop) the
    time-resolved one: (window_argmax [B, nW] int64, the power at it [B, nW]) (windowed_target_sweep)."""

    def run(sig_batch, time_vec):
        # (the non-spiking complex Beamformer has no neuron kernel, hence no time axis to pass: ref:paper_plots/target_localization.py)
        kw = dict(time_vec=time_vec) if hasattr(beamf, "tau_vec") else {}

        def one(x):
            if window is not None:
                out = beamf.localize_batch(bf_mat, x, window=window, hop=hop, **kw)
                a = out["window_argmax"].long()
                return a.cpu().numpy(), out["window_power"].gather(2, a.unsqueeze(2)).squeeze(2).cpu().numpy()
            if num_sources is not None:
                return _peaks_and_power(beamf.localize_batch(bf_mat, x, num_sources=num_sources, doa_list=doa_list,
                                                             min_separation=min_separation, rel_threshold=rel_threshold, **kw))
            return _argmax_and_power(beamf.localize_batch(bf_mat, x, **kw))

        return _in_batches(sig_batch, max_batch, one)

    return run


def _throughput_pipelined(beamf, bf_mat, time_test, sig_test, doa_all, snr_db_trial, lo, hi, batch_trials, seed, streams, scan_lane_cus,
                          ranges=None, on_done=None):
    """Trials [lo, hi) of a throughput-mode sweep with several batches in flight (runtime.StreamPipeline): batch k is synthesised
    (micloc_synth_awgn_f64: delayed template + Philox noise numbered by global trial) and localised on stream k % streams, its
    arg-max / power rows return through page-locked memory, nothing on the host waits before the end.  Long recordings (the encoder
    is time-chunked) run their serial checkpoint scans on the pipeline's scan lane.  The same bits as one batch at a time.
    `ranges`: the batches [(s0, s1), ...] to compute (default: all of [lo, hi) in steps of batch_trials -- a resumed sweep skips the
    finished ones); `on_done(s0, s1, argmax, pmax)` is called for every batch as soon as its results are known to be on the host (an
    event behind its copies, polled when the next batch is enqueued -- no extra synchronisation) and for the rest at the end.
    Returns (argmax [hi - lo] int64, pmax [hi - lo]); rows of batches that were not in `ranges` are zero."""
    import torch

    from . import runtime, synthesis
    from .snn_beamformer import neuron_impulse_response

    fs = beamf.fs
    geometry = beamf.geometry
    M = len(geometry)
    time_in, sig_in = synthesis._resample(time_test, sig_test, fs)
    tpl = runtime.Template(time_in, sig_in, fs, device=beamf.device)
    dev, T = tpl.device, tpl.T
    if ranges is None:
        ranges = [(s0, min(hi, s0 + batch_trials)) for s0 in range(lo, hi, batch_trials)]
    nplans = max(1, min(int(streams), len(ranges)))
    nir = neuron_impulse_response(time_in, beamf.tau_vec)
    plans = [beamf.plan()] + [beamf.new_plan() for _ in range(nplans - 1)]
    for pl in plans:
        pl.set_neuron_kernel(nir)
        pl.set_bf_mat(np.asarray(bf_mat, dtype=np.float64))
    G = plans[0].G
    Bmax = max(s1 - s0 for s0, s1 in ranges)
    chunked = plans[0].encoder_chunks(Bmax, T) > 1
    try:
        pipe = runtime.StreamPipeline(plans, scan_lane=scan_lane_cus if (chunked and nplans > 1) else 0)
    except (ValueError, RuntimeError):  # (MiclocError is a RuntimeError)
        # no compute-unit masks here (a partitioned device, fewer compute units per XCD than the lane wants, a driver that refuses
        # them): ordinary streams -- slower on long recordings, the same results
        pipe = runtime.StreamPipeline(plans, scan_lane=0)
    # per plan: input batch and noise workspace (a batch in flight owns them until its stream has moved on); per batch: result rows
    xs = [torch.empty((Bmax, T, M), dtype=torch.float64, device=dev) for _ in plans]
    wss = [runtime.awgn_workspace(Bmax, T, M, dev) for _ in plans]
    outs = [None] * nplans
    snr_dev = torch.from_numpy(np.ascontiguousarray(snr_db_trial[lo:hi], dtype=np.float64)).to(dev)
    am_host = torch.zeros((hi - lo,), dtype=torch.int32).pin_memory()
    pw_host = torch.zeros((hi - lo, G), dtype=torch.float64).pin_memory()
    cur = {}

    def before(i):
        s0, s1 = cur["range"]
        # delays from NumPy's cos like the host path (bit-exact with np.interp on them), one global minimum per trial (:257)
        delays = geometry.delays(doa_all[s0:s1], normalized=False)
        delays = delays - delays.min(axis=1, keepdims=True)
        d_delays = torch.from_numpy(np.ascontiguousarray(delays[:, None, :])).pin_memory().to(dev, non_blocking=True)
        runtime.synth_awgn(tpl, "apply_to_template", snr_dev[s0 - lo : s1 - lo], seed=seed, first_trial=s0, ws=wss[i], delays=d_delays,
                           out=xs[i][: s1 - s0])

    pending = []  # (event behind the batch's device -> host copies, s0, s1)

    def after(i, out):
        s0, s1 = cur["range"]
        am_host[s0 - lo : s1 - lo].copy_(out["argmax"], non_blocking=True)
        pw_host[s0 - lo : s1 - lo].copy_(out["power"], non_blocking=True)
        if on_done is not None:
            ev = torch.cuda.Event()
            ev.record()  # (on the batch's stream: StreamPipeline runs `after` under it)
            pending.append((ev, s0, s1))

    def report(all_=False):
        while pending and (all_ or pending[0][0].query()):
            _, s0, s1 = pending.pop(0)
            a = am_host[s0 - lo : s1 - lo].numpy().astype(np.int64)
            on_done(s0, s1, a, pw_host[s0 - lo : s1 - lo].numpy()[np.arange(s1 - s0), a])

    for k, (s0, s1) in enumerate(ranges):
        cur["range"] = (s0, s1)
        i = k % nplans
        if outs[i] is not None and outs[i]["argmax"].shape[0] != s1 - s0:
            outs[i] = None  # (a last, shorter batch: its own result tensors)
        pipe.snn_pipeline(lambda j: xs[j][: cur["range"][1] - cur["range"][0]], before=before, after=after, index=i, out=outs, want_power=True)
        report()
    pipe.synchronize()
    report(all_=True)
    am = am_host.numpy().astype(np.int64)
    return am, pw_host.numpy()[np.arange(hi - lo), am]


def _snr_vec(snr_db_vec):
    return np.asarray(np.linspace(-10, 20, 11) if snr_db_vec is None else snr_db_vec, dtype=np.float64)


def _sine_trials(fs, snr_db_vec, num_sim, freq_design, test_duration, snr_gain_due_to_bandwidth, band_hz=1000.0):
    """The set-up of the sine-target sweeps (target_snn_localization.py:435-449): the SNR grid (default: the scripts' 11 values), the
    `freq_design` sine of `test_duration` and the SNR of every trial, lowered by the bandwidth gain (default (fs / 2) / band_hz,
    band_hz = f_max - f_min: the paper's [1, 2] kHz band).  Returns (snr_db_vec, time_test, sig_test, snr_trial)."""
    snr_db_vec = _snr_vec(snr_db_vec)
    if snr_gain_due_to_bandwidth is None:
        snr_gain_due_to_bandwidth = (fs / 2) / band_hz
    time_test = np.arange(0, test_duration, step=1 / fs)
    sig_test = np.sin(2 * np.pi * freq_design * time_test)
    return snr_db_vec, time_test, sig_test, np.repeat(snr_db_vec - 10 * np.log10(snr_gain_due_to_bandwidth), num_sim)  # :449


def _one_doa(rand, n):
    """The truth draw of the single-target sweeps: `rand(1)[0] * 2 pi` per trial (:450)."""
    return rand(n) * 2 * np.pi


def _with_noise(synthesize):
    """Host trial of the apply_to_template sweeps (:451-457): `synthesize(truth) -> (time_in, sig [T, M])` plus white noise at the trial's
    SNR, drawn from the global stream."""

    def trial(truth, snr_db):
        time_in, sig = synthesize(truth)
        sig += np.sqrt(np.mean(sig**2)) / np.sqrt(10 ** (snr_db / 10)) * np.random.randn(*sig.shape)
        return time_in, sig

    return trial


def _monte_carlo(sweep_name, geometry, fs, doa_list, time_test, sig_test, snr_trial, seed, mode, rank, world_size, group, batch_trials,
                 out_dir, key, fields, draw, host_trial, device_batch, read_out, truth_width=(), rec=None, skip_frames=None, pipelined=None):
    """The Monte-Carlo loop of every sweep (target_snn_localization.py:447-467 / :224-245): the trials [lo, hi) of this rank in
    batches of `batch_trials`, one all-gather of the per-trial results.  Returns (truth [total, ...], the gathered fields as a dict
    name -> [total, ...], dict(exchange=..., persistence=... with out_dir)).
    The sweep's own parts:
    draw(rand, n)            the truths of n trials drawn from `rand` ([n] or [n, *truth_width]); parity mode draws one trial at a
                             time from the global stream, throughput mode all trials at once from RandomState(seed), on every rank.
    host_trial(truth, snr)   parity mode: (time_in, noisy sig [T, M]) of one trial; it consumes randn(T, M) itself.  A trial that is
                             not computed here consumes randn(skip_frames, M) instead (default: the frames of time_test resampled
                             at fs).
    device_batch(truths)     throughput mode: (time_in, noise-free x [B, T, M] on the device); the loop adds the Philox noise.
    read_out(x, time_in, truths) -> one array [B, ...] per entry of `fields`.
    fields                   (name, ShardStore column, dtype, width () or (W,), fill of the rows no run finished) per result.
    key, rec                 the sweep's ShardStore key entries (on top of the common ones below) and record dtype.
    pipelined(truth, lo, hi, ranges, on_done)  throughput mode, optional: computes all of `ranges` itself (several batches in
                             flight) and reports every batch through on_done(s0, s1, *field values).
    out_dir: per-batch result files and resume (ShardStore): finished trials are loaded, only the missing ones are computed, the
    result is the uninterrupted run's."""
    if mode not in ("parity", "throughput"):
        raise ValueError("mode must be 'parity' or 'throughput'")
    total = len(snr_trial)
    M = len(geometry)
    lo, hi = shard_range(total, rank, world_size)
    store = None
    if out_dir is not None:
        store = ShardStore(out_dir, sweep_name, total, rec=rec, seed=int(seed), mode=mode, snr_db_trial=np.asarray(snr_trial, dtype=np.float64),
                           doa_list=np.asarray(doa_list, dtype=np.float64), time_test=np.asarray(time_test, dtype=np.float64),
                           sig_test=np.asarray(sig_test, dtype=np.float64), fs=float(fs), num_mic=M,
                           r_vec=np.asarray(geometry.r_vec, dtype=np.float64), theta_vec=np.asarray(geometry.theta_vec, dtype=np.float64), **key)
    done = store.have.copy() if store is not None else np.zeros(total, dtype=bool)
    truth = np.zeros((total,) + truth_width)
    local = {name: np.full((hi - lo,) + width, fill, dtype=dtype) for name, _, dtype, width, fill in fields}
    if store is not None:  # what earlier runs finished of this rank's shard
        for name, column, *_ in fields:
            local[name][done[lo:hi]] = store.rec[column][lo:hi][done[lo:hi]]

    def finished(trials, values):
        trials = np.asarray(trials, dtype=np.int64)
        columns = {}
        for (name, column, dtype, width, _), v in zip(fields, values):
            columns[column] = np.asarray(v, dtype=dtype).reshape((len(trials),) + width)
            local[name][trials - lo] = columns[column]
        if store is not None:
            store.put(trials, truth[trials], **columns)

    def flush(x, time_in, trials):
        finished(trials, read_out(x, time_in, truth[trials]))

    if mode == "parity":
        # the reference's global MT19937 stream, replayed on every rank; a rank keeps the trials of its shard (a resumed sweep: the
        # ones of its shard that no earlier run finished -- the stream is drawn for every trial all the same)
        np.random.seed(seed)
        T = len(np.arange(np.min(time_test), np.max(time_test), step=1 / fs)) if skip_frames is None else skip_frames
        sigs, ids, time_in = [], [], None
        for trial in range(total):
            truth[trial] = draw(np.random.rand, 1)[0]
            if lo <= trial < hi and not done[trial]:
                time_in, sig = host_trial(truth[trial], snr_trial[trial])
                sigs.append(sig)
                ids.append(trial)
                if len(sigs) == batch_trials:
                    flush(np.stack(sigs), time_in, ids)
                    sigs, ids = [], []
            else:
                np.random.randn(T, M)  # keep the stream aligned: the reference draws T x M normals for every trial
        if sigs:
            flush(np.stack(sigs), time_in, ids)
    else:
        from . import synthesis

        truth[:] = draw(np.random.RandomState(seed).rand, total)  # every rank draws every trial: no dependence on the world size
        ranges = [(s0, min(hi, s0 + batch_trials)) for s0 in range(lo, hi, batch_trials)]
        ranges = [(s0, s1) for s0, s1 in ranges if not done[s0:s1].all()]  # (a batch with any trial missing is recomputed whole)
        if pipelined is not None and ranges:
            pipelined(truth, lo, hi, ranges, lambda s0, s1, *values: finished(np.arange(s0, s1), values))
        else:
            for s0, s1 in ranges:
                # noise-free array signals synthesised on the device (bit-exact with the host np.interp path), noise from the
                # Philox kernel, numbered by GLOBAL trial: the same draw for any sharding
                time_in, x = device_batch(truth[s0:s1])
                synthesis.add_noise_(x, snr_trial[s0:s1], seed=seed, first_trial=s0)
                flush(x, time_in, np.arange(s0, s1))

    # the one exchange step: every field of every trial in ONE all-gather (the truths come from the shared stream: every rank has them)
    extra = dict(exchange={})
    full = gather_shards(local, total, rank, world_size, group, stats=extra["exchange"])
    if store is not None:
        extra["persistence"] = store.stats()
    return truth, full, extra


def _one_target(beamf, time_test, sig_test):
    """The trials of the noisy-target sweep as _monte_carlo takes them (:450-457): `doa = rand(1)[0] * 2 pi`, apply_to_template on the
    host (parity mode) or on the device (throughput mode)."""
    return dict(draw=_one_doa, host_trial=_with_noise(lambda doa: synthesize_array_signal(beamf.geometry, beamf.fs, time_test, sig_test, doa)),
                device_batch=lambda doas: beamf.synthesize_batch((time_test, sig_test), doas))


def _template_sweep(beamf, bf_mat, doa_list, time_test, sig_test, snr_db_trial, num_sim, seed, mode, rank, world_size, group,
                    localizer, batch_trials, streams=4, scan_lane_cus=4, out_dir=None, sweep_name="template", store_key=None):
    """The noisy-target and the speech sweep, SNN or MUSIC (target_snn_localization.py:447-467 / :224-245): per trial
    `doa = rand(1)[0] * 2 pi`, apply_to_template at `snr_db_trial[trial]`, power, arg-max, pi-periodic error.
    Trials are processed in batches of `batch_trials` (host memory: a speech trial is 18.6 MB).  With the default localizer and
    streams > 0 the throughput mode keeps several batches in flight (_throughput_pipelined).
    store_key: the ShardStore key entries that describe the localizer (default: the hash of bf_mat)."""
    pipelined = None
    if localizer is None and streams > 0:
        # the default localizer: several batches in flight, no host synchronisation between them (same bits)
        def pipelined(doa_all, lo, hi, ranges, on_done):
            _throughput_pipelined(beamf, bf_mat, time_test, sig_test, doa_all, snr_db_trial, lo, hi, batch_trials, seed, streams, scan_lane_cus,
                                  ranges=ranges, on_done=on_done)

    localizer = localizer or device_localizer(beamf, bf_mat, max_batch=batch_trials)
    doa_all, full, extra = _monte_carlo(
        sweep_name, beamf.geometry, beamf.fs, doa_list, time_test, sig_test, snr_db_trial, seed, mode, rank, world_size, group, batch_trials, out_dir,
        key=dict(bf_mat=np.asarray(bf_mat)) if store_key is None else store_key,
        fields=(("argmax", "index", np.int64, (), 0), ("pmax", "pmax", np.float64, (), 0.0)),
        read_out=lambda x, time_in, doas: localizer(x, time_in), pipelined=pipelined, **_one_target(beamf, time_test, sig_test))
    err = doa_error(np.asarray(doa_list)[full["argmax"]], doa_all)
    shape = (len(snr_db_trial) // num_sim, num_sim)
    return dict(doa=doa_all.reshape(shape), argmax=full["argmax"].reshape(shape), pmax=full["pmax"].reshape(shape), err=err.reshape(shape),
                mae_deg=np.mean(err.reshape(shape), axis=1) * 180 / np.pi, **extra)


def noisy_target_sweep(beamf, bf_mat, doa_list, snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0, world_size=1,
                       group=None, freq_design=2000.0, test_duration=100e-3, snr_gain_due_to_bandwidth=None, localizer=None,
                       batch_trials=1100, streams=4, out_dir=None):
    """paper_plots/target_snn_localization.py:435-467.  Returns dict(doa, argmax, err, pmax: [num_snr, num_sim];
    mae_deg [num_snr]) on every rank.  out_dir: every finished batch is written there and a rerun with the same arguments resumes
    (ShardStore; `persistence` in the result says what was loaded and written)."""
    snr_db_vec, time_test, sig_test, snr_trial = _sine_trials(beamf.fs, snr_db_vec, num_sim, freq_design, test_duration, snr_gain_due_to_bandwidth)
    res = _template_sweep(beamf, bf_mat, doa_list, time_test, sig_test, snr_trial, num_sim, seed, mode, rank, world_size, group,
                          localizer, batch_trials, streams, out_dir=out_dir, sweep_name="noisy")
    res["snr_db_vec"] = snr_db_vec
    return res


def speech_source(fs, flac_path=None, pcm16=None, rate=None):
    """The speech test signal of target_snn_localization.py:148-154: the LibriSpeech utterance (FLAC file decoded by
    haghighatshoarmuir2024_amd.flac, or already-decoded int16 PCM), resampled to `fs` with np.interp on a linspace grid.
    Returns (time_fs, sig_fs)."""
    if pcm16 is None:
        from . import flac

        pcm, rate, _ = flac.decode(open(flac_path, "rb").read())
        sig = pcm[:, 0].astype(np.float64) / 32768.0  # soundfile.read returns float64 in [-1, 1)
    else:
        sig = np.asarray(pcm16).astype(np.float64) / 32768.0
    rate = int(rate)
    time_test = np.arange(len(sig)) / rate
    time_fs = np.linspace(time_test[0], time_test[-1], int(len(sig) / rate * fs))
    return time_fs, np.interp(time_fs, time_test, sig)


def speech_target_sweep(beamf, bf_mat, doa_list, source, snr_db_vec=None, num_sim=20, seed=0, mode="parity", rank=0, world_size=1,
                        group=None, localizer=None, batch_trials=None, streams=4, out_dir=None):
    """The speech accuracy sweep of paper_plots/target_snn_localization.py:213-245: `source` = (time_fs, sig_test) from
    `speech_source`, 11 SNRs x 20 trials, NO bandwidth correction of the SNR (`snr_db_target = snr_db`, :227).
    batch_trials: trials per device batch (default: 25 in parity mode -- a trial is 18.6 MB on the host --, 125 in throughput mode,
    where the batches are synthesised on the device and `streams` of them are in flight; streams=0: one batch at a time).
    out_dir: per-batch result files and resume, as in noisy_target_sweep."""
    if batch_trials is None:
        batch_trials = 125 if mode == "throughput" else 25
    snr_db_vec = _snr_vec(snr_db_vec)
    time_fs, sig_test = source
    res = _template_sweep(beamf, bf_mat, doa_list, np.asarray(time_fs, dtype=np.float64), np.asarray(sig_test, dtype=np.float64),
                          np.repeat(snr_db_vec, num_sim), num_sim, seed, mode, rank, world_size, group, localizer, batch_trials, streams,
                          out_dir=out_dir, sweep_name="speech")
    res["snr_db_vec"] = snr_db_vec
    return res


def wideband_localizer(loc, max_batch=25):
    """Localizer of the wideband sweeps: wideband.WidebandSNNLocalizer.localize_batch (filterbank, one SNN chain per band, band sum
    and arg-max on the device) -- or WidebandBeamformerLocalizer's, the complex chains of all bands as one batch -- in device batches of
    at most `max_batch` trials.  The neuron kernels are built on the live demo's own
    time axis, np.arange(T) / fs (micloc/localization_demo_snn.py:149; Demo.power_grid), not on the sweep's: the results are those of
    Demo.power_grid trial by trial, bit for bit."""

    def run(sig_batch, time_vec):
        return _in_batches(sig_batch, max_batch, lambda x: _argmax_and_power(loc.localize_batch(x)))

    return run


def _wideband_store_key(loc):
    """ShardStore key entries of a wideband localizer: the band edges (where the filterbank has them), the filterbank's coefficients,
    every band's plan key (Hilbert kernel, band-pass, robust width, polarity), tau_vec and bf_mat hash -- a resumed sweep never mixes
    band sets."""
    import hashlib

    from .runtime import pad_ba_list

    bb, aa, _ = pad_ba_list(loc.filterbank.ba_list)
    key = dict(method=type(loc).__name__, num_bands=len(loc.beamfs), fb_b=bb, fb_a=aa,
               band_edges=np.asarray(getattr(loc.filterbank, "freq_bands", np.zeros((0, 2))), dtype=np.float64))
    for f, (beamf, W) in enumerate(zip(loc.beamfs, loc.bf_mats)):
        for k, v in _method_key(beamf).items():
            if k != "method":
                key[f"band{f}_{k}"] = v
        W = np.asarray(W)  # (a complex matrix is hashed as complex128: its imaginary part is half of it)
        key[f"band{f}_bf_mat_sha256"] = hashlib.sha256(np.ascontiguousarray(W, dtype=np.complex128 if np.iscomplexobj(W) else np.float64).tobytes()).hexdigest()
    return key


def wideband_speech_sweep(loc, doa_list, source, snr_db_vec=None, num_sim=20, seed=0, mode="parity", rank=0, world_size=1, group=None,
                          localizer=None, batch_trials=None, out_dir=None):
    """The speech accuracy sweep (speech_target_sweep: paper_plots/target_snn_localization.py:213-245, 11 SNRs x 20 trials, no bandwidth
    correction) read out by the WIDEBAND localizer `loc` (wideband.WidebandSNNLocalizer: the live demo's filterbank + per-band chains +
    band sum, micloc/localization_demo_snn.py:125-193; or wideband.WidebandBeamformerLocalizer, the complex Beamformer's form of it,
    micloc/localization_demo.py:158-182) instead of one band.  One batch at a time (the band pipeline runs on one
    stream).  `localizer`: another read-out with wideband_localizer's signature (tests).  out_dir: resume as in noisy_target_sweep; the
    store key carries the band edges, the filterbank coefficients and every band's parameters and bf_mat hash."""
    if batch_trials is None:
        batch_trials = 125 if mode == "throughput" else 25
    snr_db_vec = _snr_vec(snr_db_vec)
    time_fs, sig_test = source
    res = _template_sweep(loc.beamfs[0], None, doa_list, np.asarray(time_fs, dtype=np.float64), np.asarray(sig_test, dtype=np.float64),
                          np.repeat(snr_db_vec, num_sim), num_sim, seed, mode, rank, world_size, group,
                          localizer or wideband_localizer(loc, max_batch=batch_trials), batch_trials, 0, out_dir=out_dir,
                          sweep_name="wideband-speech", store_key=_wideband_store_key(loc))
    res["snr_db_vec"] = snr_db_vec
    return res


def parse_bands(text):
    """`--bands 1000:1600,1600:2400,2400:3400` -> [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]] (Hz, low:high per band)."""
    bands = []
    for part in str(text).split(","):
        try:
            lo, hi = (float(v) for v in part.split(":"))
        except ValueError:
            raise ValueError(f"--bands takes low:high pairs separated by commas, got {part!r}")
        if not 0 < lo < hi:
            raise ValueError(f"a band needs 0 < low < high, got {part!r}")
        bands.append([lo, hi])
    if not 1 <= len(bands) <= 16:
        raise ValueError(f"1 .. 16 bands, got {len(bands)}")
    return bands


def music_localizer(music, num_active_freq, duration_overlap, num_fft_bin, max_batch=100, num_sources=None, min_separation=None, rel_threshold=0.0):
    """Localizer of the MUSIC sweeps: MUSIC.localize_batch (the scripts' read-out power = mean_s |P|^2, arg-max) in device batches
    of at most `max_batch` trials; the [B, S, G] spectra stay in the workspace.  With num_sources=K: (peaks [B, K] int64,
    peak_power [B, K]) instead (multi_target_sweep)."""

    def one(x):
        if num_sources is not None:
            return _peaks_and_power(music.localize_batch(x, num_active_freq, duration_overlap, num_fft_bin, want_spectrum=False,
                                                         num_sources=num_sources, min_separation=min_separation, rel_threshold=rel_threshold))
        return _argmax_and_power(music.localize_batch(x, num_active_freq, duration_overlap, num_fft_bin, want_spectrum=False))

    return lambda sig_batch, time_vec: _in_batches(sig_batch, max_batch, one)


def _music_store_key(music, num_active_freq, duration_overlap, num_fft_bin):
    return dict(freq_range=np.asarray(music.freq_range, dtype=np.float64), num_fft_bin=int(num_fft_bin), num_active_freq=int(num_active_freq),
                duration_overlap=float(duration_overlap), frame_duration=float(music.frame_duration), speed=float(music.geometry.speed))


def music_noisy_sweep(music, snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0, world_size=1, group=None, num_active_freq=1,
                      num_fft_bin=2048, duration_overlap=0.0, freq_design=2000.0, test_duration=1000e-3, snr_gain_due_to_bandwidth=None,
                      batch_trials=100, out_dir=None):
    """The noisy-target MUSIC sweep of paper_plots/target_localization_MUSIC.py (test_noisy_target, statistical part): a 1 s
    `freq_design` sine, 11 SNRs x num_sim trials, SNR lowered by 10 log10((fs/2) / (f_max - f_min)), per trial `doa = rand(1)[0] * 2 pi`,
    apply_to_template (k = 1, N = 2048, no overlap), power = mean_s |P|^2, arg-max, arcsin|sin(err)|.  `music` is a MUSIC (the script's:
    7-mic circular array, band [1600, 2400], 57 DoAs, frame_duration 1.0).  Modes, sharding and out_dir resume as noisy_target_sweep;
    the ShardStore key also covers band, N, k, overlap and frame duration."""
    f_min, f_max = music.freq_range
    snr_db_vec, time_test, sig_test, snr_trial = _sine_trials(music.fs, snr_db_vec, num_sim, freq_design, test_duration, snr_gain_due_to_bandwidth,
                                                              band_hz=f_max - f_min)
    loc = music_localizer(music, num_active_freq, duration_overlap, num_fft_bin, max_batch=batch_trials)
    res = _template_sweep(music, None, music.doa_list, time_test, sig_test, snr_trial, num_sim, seed, mode, rank, world_size, group, loc,
                          batch_trials, 0, out_dir=out_dir, sweep_name="music-noisy",
                          store_key=_music_store_key(music, num_active_freq, duration_overlap, num_fft_bin))
    res["snr_db_vec"] = snr_db_vec
    return res


def music_speech_sweep(music, source, snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0, world_size=1, group=None, num_active_freq=1,
                       num_fft_bin=2048, duration_overlap=0.0, batch_trials=25, out_dir=None):
    """The speech-target MUSIC sweep of paper_plots/target_localization_MUSIC.py (test_speech_target, statistical part): `source` =
    (time_fs, sig_test) from `speech_source`, 11 SNRs x num_sim trials, NO bandwidth correction, k = 1, N = 2048 (the script's MUSIC:
    449 DoAs, frame_duration 1.0: 7 slices per trial).  Modes, sharding and out_dir resume as music_noisy_sweep."""
    snr_db_vec = _snr_vec(snr_db_vec)
    time_fs, sig_test = source
    loc = music_localizer(music, num_active_freq, duration_overlap, num_fft_bin, max_batch=batch_trials)
    res = _template_sweep(music, None, music.doa_list, np.asarray(time_fs, dtype=np.float64), np.asarray(sig_test, dtype=np.float64),
                          np.repeat(snr_db_vec, num_sim), num_sim, seed, mode, rank, world_size, group, loc, batch_trials, 0, out_dir=out_dir,
                          sweep_name="music-speech", store_key=_music_store_key(music, num_active_freq, duration_overlap, num_fft_bin))
    res["snr_db_vec"] = snr_db_vec
    return res


def _xylo_win_size(doa_list):
    """find_peak_location's window of the Xylo sweeps (target_xylo_localization.py:600-603)."""
    return 2 * ((len(doa_list) // 32) // 2) + 1


def _xylo_trials(demo, snr_db_vec, num_sim, test_duration, snr_gain_due_to_bandwidth, device_delays):
    """The trials of the Xylo sweeps (target_xylo_localization.py:549-560, :575-588): the chirp over the design band, `signal_from_template`
    at the drawn DoA plus white noise.  Returns dict(geometry, fs, snr_db_vec, time_test, sig_test, snr_trial, frames and mc, the draw /
    host_trial / device_batch / skip_frames entries of _monte_carlo)."""
    from . import synthesis
    from .xylo_snn_localization import signal_from_template

    fs = demo.fs
    snr_db_vec = _snr_vec(snr_db_vec)
    f_min, f_max = [float(v) for v in demo.freq_bands[0]]
    if snr_gain_due_to_bandwidth is None:
        snr_gain_due_to_bandwidth = (fs / 2) / (f_max - f_min)
    time_test = np.arange(0, test_duration, step=1 / fs)
    period = time_test[-1]
    freq_inst = f_min + (f_max - f_min) * (time_test % period) / period
    sig_test = np.sin(2 * np.pi * np.cumsum(freq_inst) * 1 / fs)
    geometry = demo.beamfs[0].geometry
    snr_trial = np.repeat(snr_db_vec - 10 * np.log10(snr_gain_due_to_bandwidth), num_sim)

    def host_trial(doa, snr_db):
        sig = signal_from_template(geometry, (time_test, sig_test, doa))
        noise_sigma = np.sqrt(np.mean(sig**2) / 10 ** (snr_db / 10))
        return None, sig + noise_sigma * np.random.randn(*sig.shape)

    mc = dict(draw=_one_doa, host_trial=host_trial, skip_frames=len(time_test),
              device_batch=lambda doas: (None, synthesis.signal_from_template_batch(geometry, (time_test, sig_test), doas, device=demo.device,
                                                                                    device_delays=device_delays)))
    return dict(geometry=geometry, fs=fs, snr_db_vec=snr_db_vec, time_test=time_test, sig_test=sig_test, snr_trial=snr_trial,
                frames=len(time_test), mc=mc)


def xylo_target_sweep(demo, snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0, world_size=1, group=None,
                      test_duration=1000e-3, snr_gain_due_to_bandwidth=None, batch_trials=None, device_delays=None, peak=None, out_dir=None):
    """The Xylo accuracy sweep of paper_plots/target_xylo_localization.py:540-608 (and its `_unipolar` twin): chirp test
    signal over the design band (:549-560), per trial `signal_from_template` -> AWGN -> `spike_encoding` -> `xylo_process`
    -> spike rate -> `find_peak_location(win_size)` with win_size = 2 * ((num_grid // 32) // 2) + 1 (:600-603) -> error.

    PARITY UNPINNED for the integer-LIF stage (rockpool / XyloSim absent: xylo_snn_localization.py module docstring);
    everything around it follows the reference's arithmetic.  `demo` is a xylo_snn_localization.Demo with one band.
    batch_trials: trials per device batch -- default 50 in parity mode (host arrays of 2.7 MB per trial), 1100 in throughput mode: the
    integer LIF is one serial chain per trial, a launch takes as long for 50 trials as for 1100."""
    from .utils import find_peak_location

    doa_list = demo.doa_list
    win_size = _xylo_win_size(doa_list)
    if batch_trials is None:
        batch_trials = 1100 if mode == "throughput" else 50
    if device_delays is None:
        device_delays = mode == "throughput"
    if peak is None:
        peak = "device" if mode == "throughput" else "host"
    tr = _xylo_trials(demo, snr_db_vec, num_sim, test_duration, snr_gain_due_to_bandwidth, device_delays)
    geometry, fs, snr_db_vec, time_test, sig_test, snr_trial = (tr[k] for k in ("geometry", "fs", "snr_db_vec", "time_test", "sig_test", "snr_trial"))

    def read_out(x, time_in, doas):
        if peak == "device":  # find_peak_location on the device (exact integer window sums): only indices come back
            idx = demo.peak_batch(x, win_size).cpu().numpy().astype(np.int64)
            demo.network().check()  # (the copy above synchronised: a broken ticket-queue launch raises here)
            return (idx,)
        rate = demo.rate_batch(x).cpu().numpy()  # [B, G]: mean(spikes_out) * fs per DoA
        demo.network().check()
        idx = []
        for p in rate:
            mx = p.max()
            p = p / mx if mx > 0 else p  # :595 (an all-silent output divides 0 by 0 in the reference)
            idx.append(int(find_peak_location(sig_in=p, win_size=win_size)))
        return (idx,)

    # (the record's `pmax` stays zero: this sweep keeps the peak index alone; a skipped trial consumes the frames of time_test itself)
    doa_all, full, extra = _monte_carlo(
        "xylo", geometry, fs, doa_list, time_test, sig_test, snr_trial, seed, mode, rank, world_size, group, batch_trials, out_dir,
        key=dict(bf_mat=np.asarray(demo.bf_mats[0]), bipolar=bool(demo.bipolar_spikes), peak=peak, device_delays=bool(device_delays),
                 win_size=int(win_size)),
        fields=(("index", "index", np.int64, (), 0),), read_out=read_out, **tr["mc"])
    del extra["exchange"]  # (this sweep's result has never reported its exchange)
    err = doa_error(np.asarray(doa_list)[full["index"]], doa_all)
    shape = (len(snr_db_vec), num_sim)
    return dict(doa=doa_all.reshape(shape), index=full["index"].reshape(shape), err=err.reshape(shape),
                mae_deg=np.mean(err.reshape(shape), axis=1) * 180 / np.pi, snr_db_vec=snr_db_vec, win_size=win_size, parity="unpinned (integer LIF)",
                **extra)


# ---- multi-target sweep ---------------------------------------------------------------------------------------------------------

def _method_key(beamf):
    """ShardStore key entries for the localizer's own parameters: its class, for the beamformers the plan key (Hilbert kernel,
    band-pass b / a, robust width, bipolar) and tau_vec, for MUSIC its band, frame duration, DoA grid and speed of sound (the
    per-call parameters k, N and overlap come with store_key, _music_store_key)."""
    key = dict(method=type(beamf).__name__)
    if hasattr(beamf, "kernel"):
        key["kernel"] = np.asarray(beamf.kernel, dtype=np.float64)
    if hasattr(beamf, "bandpass_filter"):
        b, a = beamf.bandpass_filter
        key["iir_b"], key["iir_a"] = np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64)
    if hasattr(beamf, "spk_encoder"):
        key["robust_width"], key["bipolar"] = int(beamf.spk_encoder.robust_width), bool(beamf.spk_encoder.bipolar)
    if hasattr(beamf, "tau_vec"):
        key["tau_vec"] = np.asarray(beamf.tau_vec, dtype=np.float64)
    if hasattr(beamf, "frame_duration"):  # MUSIC: band, frame length, DoA grid of the steering table, speed of sound
        key["freq_range"] = np.asarray(beamf.freq_range, dtype=np.float64)
        key["frame_duration"] = float(beamf.frame_duration)
        key["music_doa_list"] = np.asarray(beamf.doa_list, dtype=np.float64)
        key["speed"] = float(beamf.geometry.speed)
    return key


def _localizer_key(beamf, bf_mat, store_key):
    """ShardStore key entries of a sweep's localizer: bf_mat (where there is one), the method's own parameters, then store_key."""
    return {**({} if bf_mat is None else dict(bf_mat=np.asarray(bf_mat))), **_method_key(beamf), **(store_key or {})}


def _draw_doas(draw, K, min_separation, max_redraws):
    """`draw(K) * 2 pi`, drawn again while two targets are closer than min_separation in the pi-periodic error."""
    doa = draw(K) * 2 * np.pi
    for _ in range(max_redraws):
        if K < 2 or min(doa_error(doa[i], doa[j]) for i in range(K) for j in range(i + 1, K)) >= min_separation:
            return doa
        doa = draw(K) * 2 * np.pi
    raise ValueError(f"no {K} DoAs at least {min_separation} rad apart in {max_redraws} redraws")


def synthesize_targets(geometry, fs, time_test, sig_test, doas, gains):
    """Noise-free array signal of K constant-DoA targets on the host: every copy is delayed as apply_to_template delays it, with ONE
    shift (the minimum over all targets' delays), scaled by its gain and summed `sig = 0; sig += g_k * copy_k` in k order.
    Returns (time_in [T], sig [T, M])."""
    time_test = np.asarray(time_test, dtype=np.float64)
    time_in = np.arange(time_test.min(), time_test.max(), step=1 / fs)
    sig_in = np.interp(time_in, time_test, np.asarray(sig_test, dtype=np.float64))
    delays = np.stack([geometry.delays(float(d), normalized=False) for d in doas])  # [K, M]
    delays = delays - delays.min()
    sig = np.zeros((len(time_in), delays.shape[1]))
    for k in range(len(doas)):
        t = time_in.reshape(1, -1) - delays[k].reshape(-1, 1)
        np.maximum(t, time_in.min(), out=t)
        sig += gains[k] * np.interp(t.ravel(), time_in, sig_in).reshape(t.shape).T
    return time_in, sig


def synthesize_targets_batch(geometry, fs, time_test, sig_test, doas, gains, device=None):
    """synthesize_targets for a batch of trials on the device (micloc_synth_targets_f64, APPLY_TO_TEMPLATE, host delays: the same
    bits).  doas [B, K] -> (time_in [T], x [B, T, M] device tensor)."""
    from . import runtime, synthesis

    doas = np.asarray(doas, dtype=np.float64)
    B, K = doas.shape
    time_in, sig_in = synthesis._resample(time_test, sig_test, fs)
    tpl = runtime.Template(time_in, sig_in, fs, device=device)
    delays = geometry.delays(doas.ravel(), normalized=False).reshape(B, K, -1)
    delays = delays - delays.min(axis=(1, 2), keepdims=True)
    gains = np.asarray(gains, dtype=np.float64)
    gain = None
    if not np.all(gains == 1.0):  # (1 * r is r: no table for unit gains)
        # the kernel reads gain [B, K, T]: expanded on the device, only K numbers cross PCIe
        gain = runtime._as_dev(gains, tpl.device).reshape(1, K, 1).expand(B, K, tpl.T).contiguous()
    return time_in, runtime.synth_targets(tpl, "apply_to_template", delays=delays, gain=gain)


def match_errors(doa_true, doa_list, index):
    """Matched pi-periodic errors of K estimates against K true DoAs: doa_true [N, K], index [N, K] (-1: no peak) -> err [N, K],
    err[n, k] = the error of truth k under the permutation of the estimates with the least summed error (ties: the first permutation
    in lexicographic order).  A missing peak costs pi / 2, the metric's maximum."""
    import itertools

    doa_list = np.asarray(doa_list, dtype=np.float64)
    N, K = index.shape
    est = doa_list[np.maximum(index, 0)]
    best = best_sum = None
    for perm in itertools.permutations(range(K)):
        e = np.where(index[:, perm] >= 0, doa_error(est[:, perm], doa_true), np.pi / 2)
        tot = e[:, 0].copy()
        for k in range(1, K):
            tot += e[:, k]
        if best is None:
            best, best_sum = e, tot
        else:
            better = tot < best_sum
            best[better], best_sum[better] = e[better], tot[better]
    return best


def multi_target_sweep(beamf, bf_mat, doa_list, num_targets=2, min_separation=np.pi / 4, gains=None, peak_separation=None, tol=None,
                       rel_threshold=0.0, snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0, world_size=1, group=None,
                       freq_design=2000.0, test_duration=100e-3, snr_gain_due_to_bandwidth=None, localizer=None, batch_trials=1100,
                       out_dir=None, store_key=None, max_redraws=10_000):
    """The noisy-target sweep with K = num_targets simultaneous targets of the same `freq_design` sine.  Per trial: `doa = rand(K) * 2 pi`,
    drawn again while two targets are closer than `min_separation` in the pi-periodic error (parity mode: the global MT19937 stream,
    then randn(T, M) of the noise; throughput mode: RandomState(seed) for every trial on every rank, noise from the Philox kernel by
    global trial); the array signal sums the K delayed copies with `gains` (synthesize_targets); noise as apply_to_template from
    the summed signal's power; localize with num_sources=K (peaks at least `peak_separation` apart, `rel_threshold`); estimates
    are matched to truths by the permutation with the least summed pi-periodic error (match_errors).
    `localizer(sig_batch, time_vec) -> (index [B, K], value [B, K])` replaces the device pipeline (default: device_localizer with
    num_sources; MUSIC: music_localizer with num_sources).  Defaults: min_separation 45 deg, gains 1, peak_separation and tol
    min_separation / 2.  At num_targets = 1 this is noisy_target_sweep, bit for bit, in both modes.
    Returns dict(doa, peaks, peak_power, err: [num_snr, num_sim, K]; mae_deg (over trials and targets) and resolved_rate (all K
    peaks found, every matched error <= tol): [num_snr]).  Sharding, the one exchange and out_dir resume as noisy_target_sweep;
    the ShardStore key also covers K, both separations, tol, gains, rel_threshold and the method's parameters (store_key adds to it)."""
    K = int(num_targets)
    if not 1 <= K <= 4:
        raise ValueError("num_targets must be between 1 and 4")
    min_separation = float(min_separation)
    if not (min_separation >= 0.0 and K * min_separation < np.pi):
        raise ValueError(f"{K} targets cannot be {min_separation} rad apart in the pi-periodic error: need K * min_separation < pi")
    gains = np.ones(K) if gains is None else np.asarray(gains, dtype=np.float64).reshape(-1)
    if len(gains) != K:
        raise ValueError(f"gains has {len(gains)} entries for {K} targets")
    peak_separation = min_separation / 2 if peak_separation is None else float(peak_separation)
    tol = min_separation / 2 if tol is None else float(tol)
    doa_list = np.asarray(doa_list, dtype=np.float64)
    fs, geometry = beamf.fs, beamf.geometry
    snr_db_vec, time_test, sig_test, snr_trial = _sine_trials(fs, snr_db_vec, num_sim, freq_design, test_duration, snr_gain_due_to_bandwidth)
    if localizer is None:
        localizer = device_localizer(beamf, bf_mat, max_batch=batch_trials, num_sources=K, doa_list=doa_list, min_separation=peak_separation,
                                     rel_threshold=rel_threshold)
    # (a trial no run finished reads -1 / NaN: "no peak"; at K = 1 the draws are the noisy sweep's, one rand(1) per trial)
    doa_all, full, extra = _monte_carlo(
        "multi-noisy", geometry, fs, doa_list, time_test, sig_test, snr_trial, seed, mode, rank, world_size, group, batch_trials, out_dir,
        key=dict(num_targets=K, min_separation=min_separation, peak_separation=peak_separation, tol=tol, gains=gains,
                 rel_threshold=float(rel_threshold), **_localizer_key(beamf, bf_mat, store_key)),
        rec=[("trial", "<i8"), ("doa", "<f8", (K,)), ("index", "<i8", (K,)), ("pmax", "<f8", (K,))],
        fields=(("peaks", "index", np.int64, (K,), -1), ("peak_power", "pmax", np.float64, (K,), np.nan)), truth_width=(K,),
        draw=lambda rand, n: np.stack([_draw_doas(rand, K, min_separation, max_redraws) for _ in range(n)]),
        host_trial=_with_noise(lambda doas: synthesize_targets(geometry, fs, time_test, sig_test, doas, gains)),
        device_batch=lambda doas: synthesize_targets_batch(geometry, fs, time_test, sig_test, doas, gains, device=getattr(beamf, "device", None)),
        read_out=lambda x, time_in, doas: localizer(x, time_in))
    peaks = full["peaks"]
    err = match_errors(doa_all, doa_list, peaks)
    tol_ok = np.all((peaks >= 0) & (err <= tol), axis=1)
    S = len(snr_db_vec)
    return dict(doa=doa_all.reshape(S, num_sim, K), peaks=peaks.reshape(S, num_sim, K), peak_power=full["peak_power"].reshape(S, num_sim, K),
                err=err.reshape(S, num_sim, K), mae_deg=np.mean(err.reshape(S, num_sim * K), axis=1) * 180 / np.pi,
                resolved_rate=np.mean(tol_ok.reshape(S, num_sim), axis=1), snr_db_vec=snr_db_vec, **extra)


def median_window_index(doa_list, index):
    """The median-over-windows estimate of every trial: index [N, nW] -> [N], the window estimate with the least summed pi-periodic
    error (doa_error, the sweep's metric) to the trial's other window estimates -- the median of a sample on the half circle, where
    sorting has no meaning at the seam; ties go to the earlier window.  One window: that window's estimate."""
    doa_list = np.asarray(doa_list, dtype=np.float64)
    index = np.asarray(index, dtype=np.int64)
    est = doa_list[index]  # [N, nW]
    cost = np.zeros(est.shape)
    for m in range(est.shape[1]):
        cost += doa_error(est, est[:, m : m + 1])
    return index[np.arange(len(index)), np.argmin(cost, axis=1)]


def windowed_target_sweep(beamf, bf_mat, doa_list, window, hop=None, snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0,
                          world_size=1, group=None, freq_design=2000.0, test_duration=100e-3, snr_gain_due_to_bandwidth=None,
                          localizer=None, batch_trials=1100, out_dir=None, store_key=None, trials=None):
    """The noisy-target sweep with the time-resolved read-out: the trials of noisy_target_sweep (the same draws in both modes),
    every one localised per window of `window` frames every `hop` frames (default: `window`; utils.window_bounds, hop <= window so
    that every window holds frames; the device wants multiples of plan().window_quantum()).
    `localizer(sig_batch, time_vec) -> (index [B, nW], value [B, nW])` replaces the device pipeline (default: device_localizer with
    window / hop).  Returns dict(doa [num_snr, num_sim]; window_argmax, window_pmax, window_err [num_snr, num_sim, nW];
    window_mae_deg [num_snr, nW], the MAE per SNR and window; window_start [nW]; and of the median-over-windows estimate
    (median_window_index) argmax, pmax (the power of the window that gave it), err [num_snr, num_sim] and mae_deg [num_snr]).  With
    window >= T there is one window and argmax, pmax, err, mae_deg are noisy_target_sweep's, bit for bit.
    Sharding, the one exchange and out_dir resume as noisy_target_sweep; the ShardStore key also covers window, hop, the record
    width nW and the method's parameters (class, plan key, tau_vec; store_key adds to it, e.g. a tag for an injected localizer).
    trials: another test signal and synthesis in place of the sine trials (_xylo_trials' dict: snr_db_vec, time_test, sig_test, snr_trial,
    the `frames` of a trial and `mc`, _monte_carlo's draw / host_trial / device_batch entries); freq_design, test_duration and
    snr_gain_due_to_bandwidth then belong to whoever made it."""
    from .utils import window_bounds

    window = int(window)
    hop = window if hop is None else int(hop)
    if window < 1 or hop < 1:
        raise ValueError("window and hop must be at least 1 frame")
    if hop > window:
        raise ValueError("the windowed sweep needs hop <= window (a window past the recording would hold no frame)")
    doa_list = np.asarray(doa_list, dtype=np.float64)
    fs = beamf.fs
    if trials is None:
        snr_db_vec, time_test, sig_test, snr_trial = _sine_trials(fs, snr_db_vec, num_sim, freq_design, test_duration, snr_gain_due_to_bandwidth)
        frames, mc = len(np.arange(time_test.min(), time_test.max(), step=1 / fs)), _one_target(beamf, time_test, sig_test)
    else:
        snr_db_vec, time_test, sig_test, snr_trial, frames, mc = (trials[k] for k in ("snr_db_vec", "time_test", "sig_test", "snr_trial", "frames", "mc"))
    total = len(snr_trial)
    start, _ = window_bounds(frames, window, hop)
    nW = len(start)
    if localizer is None:
        localizer = device_localizer(beamf, bf_mat, max_batch=batch_trials, window=window, hop=hop)
    doa_all, full, extra = _monte_carlo(
        "windowed-noisy", beamf.geometry, fs, doa_list, time_test, sig_test, snr_trial, seed, mode, rank, world_size, group, batch_trials, out_dir,
        key=dict(record_width=nW, window=window, hop=hop, **_localizer_key(beamf, bf_mat, store_key)),
        rec=[("trial", "<i8"), ("doa", "<f8"), ("index", "<i8", (nW,)), ("pmax", "<f8", (nW,))],
        fields=(("index", "index", np.int64, (nW,), 0), ("value", "pmax", np.float64, (nW,), 0.0)),
        read_out=lambda x, time_in, doas: localizer(x, time_in), **mc)
    w_index, w_value = full["index"], full["value"]
    w_err = doa_error(doa_list[w_index], doa_all[:, None])
    med = median_window_index(doa_list, w_index)
    med_window = np.argmax(w_index == med[:, None], axis=1)  # (the first window that gave the median estimate)
    err = doa_error(doa_list[med], doa_all)
    S = len(snr_db_vec)
    shape = (S, num_sim)
    return dict(doa=doa_all.reshape(shape), window_argmax=w_index.reshape(S, num_sim, nW), window_pmax=w_value.reshape(S, num_sim, nW),
                window_err=w_err.reshape(S, num_sim, nW), window_mae_deg=np.mean(w_err.reshape(S, num_sim, nW), axis=1) * 180 / np.pi,
                window_start=start, argmax=med.reshape(shape), pmax=w_value[np.arange(total), med_window].reshape(shape), err=err.reshape(shape),
                mae_deg=np.mean(err.reshape(shape), axis=1) * 180 / np.pi, snr_db_vec=snr_db_vec, **extra)


def moving_doa_path(time_vec, duration, doa_max, num_period, phase):
    """The DoA of the moving target at the times of `time_vec`: doa_max * sin(num_period * pi * t / duration + phase)
    (paper_plots/target_snn_localization.py:595-597 with a start phase; phase [B] -> [B, T])."""
    t = np.asarray(time_vec, dtype=np.float64)
    ph = np.asarray(phase, dtype=np.float64)
    return doa_max * np.sin(num_period * np.pi * t / duration + ph[..., None])


def track_errors(doa_list, index, doa_true, lag_frames, settle_frames):
    """Per-trial tracking errors: index [B, T] (the estimate per frame: a device tensor or an array), doa_true [B, T] (NumPy) ->
    (mean [B], median [B]) of arcsin|sin(doa_list[index[:, t]] - doa_true[:, t - lag_frames])| over the frames
    t >= max(settle_frames, lag_frames).  A device tensor is reduced on the device (only the 2 B scalars come back)."""
    T = doa_true.shape[1]
    t0 = max(int(settle_frames), int(lag_frames))
    lag = int(lag_frames)
    if not 0 <= t0 < T:
        raise ValueError(f"no frame to score: settle_frames / lag_frames {t0} of {T} frames")
    truth = np.ascontiguousarray(doa_true[:, t0 - lag : T - lag])
    if type(index).__module__.startswith("torch"):
        import torch

        dl = torch.as_tensor(np.asarray(doa_list, dtype=np.float64), device=index.device)
        e = torch.asin(torch.abs(torch.sin(dl[index[:, t0:].long()] - torch.as_tensor(truth, device=index.device))))
        return e.mean(dim=1).cpu().numpy(), e.quantile(0.5, dim=1).cpu().numpy()
    e = doa_error(np.asarray(doa_list, dtype=np.float64)[np.asarray(index)[:, t0:]], truth)
    return e.mean(axis=1), np.median(e, axis=1)


def track_localizer(beamf, bf_mat, envelope, max_batch=1100):
    """Default localizer of moving_target_sweep: the fused tracking call (track_batch); index [B, T] stays on the device."""

    def run(sig_batch, time_vec):
        kw = dict(time_vec=time_vec) if hasattr(beamf, "tau_vec") else {}
        return _in_batches(sig_batch, max_batch, lambda x: (beamf.track_batch(bf_mat, x, envelope, **kw)["index"],))[0]

    return run


def _wrap_rows(x, half):
    """np.roll(x, half, axis=1)[:, :half] of a complete batch [B, T, M] (array or device tensor), zero rows behind a recording shorter
    than `half`: the wrap_tail of a stream that is to reproduce the one-shot call."""
    if isinstance(x, np.ndarray):
        from .streaming import ComplexStreamingLocalizer

        return ComplexStreamingLocalizer.wrap_rows(x, 2 * half)
    import torch

    out = torch.zeros((x.shape[0], half, x.shape[2]), dtype=x.dtype, device=x.device)
    k = min(half, x.shape[1])
    out[:, :k, :] = torch.roll(x, half, dims=1)[:, :k, :]
    return out


def stream_track_localizer(beamf, bf_mat, envelope, tile, max_batch=1100):
    """track_localizer's place in moving_target_sweep(localizer=) for audio that arrives while it is tracked: every batch is pushed in
    tiles of `tile` frames through a tracked stream (beamf.streaming_localizer(track=envelope); an SNN stream takes multiples of 16) and
    the index [B, T] of finish() comes back -- the bits of track_batch on the whole batch, which the wrap-around rows of np.roll (known
    here: the batch is complete) and the one-shot call's time axis of the neuron kernel make possible."""
    tile = int(tile)
    if tile < 1:
        raise ValueError("tile must be at least 1 frame")
    snn = hasattr(beamf, "tau_vec")
    half = len(beamf.kernel) // 2

    def run(sig_batch, time_vec):
        def one(x):
            B, T, _ = x.shape
            kw = dict(time_vec=time_vec) if snn else {}
            s = beamf.streaming_localizer(bf_mat, batch=B, total_frames=T, wrap_tail=_wrap_rows(x, half), max_tile=min(tile, T), track=envelope, **kw)
            for t in range(0, T, tile):
                s.push(x[:, t : t + tile, :])
            return (s.finish()["track_index"],)

        return _in_batches(sig_batch, max_batch, one)[0]

    return run


def stream_multi_localizer(beamf, bf_mat, doa_list, tile, num_sources, min_separation=None, rel_threshold=0.0, max_batch=1100):
    """device_localizer(num_sources=)'s place in multi_target_sweep(localizer=) for audio that arrives while it is localised: every batch is
    pushed in tiles of `tile` frames through a stream built with num_sources (beamf.streaming_localizer(num_sources=, doa_list=); an SNN
    stream takes multiples of 16) and finish()'s (peaks [B, K] int64, peak_power [B, K]) come back -- the bits of
    localize_batch(num_sources=) on the whole batch, which the wrap-around rows of np.roll (known here: the batch is complete) and the
    one-shot call's time axis of the neuron kernel make possible."""
    tile = int(tile)
    if tile < 1:
        raise ValueError("tile must be at least 1 frame")
    snn = hasattr(beamf, "tau_vec")
    half = len(beamf.kernel) // 2

    def run(sig_batch, time_vec):
        def one(x):
            B, T, _ = x.shape
            kw = dict(time_vec=time_vec) if snn else {}
            s = beamf.streaming_localizer(bf_mat, batch=B, total_frames=T, wrap_tail=_wrap_rows(x, half), max_tile=min(tile, T),
                                          num_sources=num_sources, doa_list=doa_list, min_separation=min_separation, rel_threshold=rel_threshold, **kw)
            for t in range(0, T, tile):
                s.push(x[:, t : t + tile, :])
            return _peaks_and_power(s.finish())

        return _in_batches(sig_batch, max_batch, one)

    return run


def moving_target_sweep(beamf, bf_mat, doa_list, envelope, doa_max=np.pi / 2, num_period=0.5, lag_frames=None, settle_frames=None,
                        snr_db_vec=None, num_sim=100, seed=0, mode="parity", rank=0, world_size=1, group=None, freq_design=2000.0,
                        test_duration=100e-3, snr_gain_due_to_bandwidth=None, localizer=None, batch_trials=1100, out_dir=None, store_key=None):
    """The noisy-target sweep with a MOVING target and the per-frame read-out (paper_plots/target_snn_localization.py:585-628,
    `test_moving_target`): the test signal and SNR grid of noisy_target_sweep; per trial the DoA follows
    `doa_max * sin(num_period * pi * t / duration + phase)` (moving_doa_path) with `phase = rand(1)[0] * 2 pi` drawn where the noisy sweep
    draws its DoA (parity mode: the global MT19937 stream, `rand(1)` then `randn(T, M)`; throughput mode: RandomState(seed) for all
    trials on every rank, device synthesis with moving delays and Philox noise by global trial).  The estimate of frame t,
    `doa_list[index[t]]` with index = argmax_g Envelope(y)[t, g], is scored against the truth of frame t - lag_frames (default
    int(kernel_duration * fs), the script's alignment at :628) over the frames t >= settle_frames (default int(fs * fall_time)) by the
    pi-periodic error (track_errors: on the device; only per-trial scalars are gathered, in one all-gather).
    `localizer(sig_batch, time_vec) -> index [B, T]` (device tensor or array) replaces the fused call (track_localizer), e.g. by the
    tracked stream (stream_track_localizer).
    Returns dict(phase, err (mean error over frames), med (median over frames): [num_snr, num_sim]; track_mae_deg [num_snr], the mean of
    err over trials; track_median_deg [num_snr], the median over trials of med; mae_deg = track_mae_deg).  out_dir resume as the other
    sweeps; the key also covers doa_max, num_period, lag_frames, settle_frames, the envelope's window lengths and the method's
    parameters (class, plan key, tau_vec; store_key adds to it, e.g. a tag for an injected localizer)."""
    doa_list = np.asarray(doa_list, dtype=np.float64)
    fs, geometry = beamf.fs, beamf.geometry
    snr_db_vec, time_test, sig_test, snr_trial = _sine_trials(fs, snr_db_vec, num_sim, freq_design, test_duration, snr_gain_due_to_bandwidth)
    time_in = np.arange(time_test.min(), time_test.max(), step=1 / fs)
    T = len(time_in)
    lag_frames = int(beamf.kernel_duration * fs) if lag_frames is None else int(lag_frames)
    settle_frames = int(fs * envelope.fall_time) if settle_frames is None else int(settle_frames)
    if lag_frames < 0 or settle_frames < 0 or max(lag_frames, settle_frames) >= T:
        raise ValueError(f"lag_frames ({lag_frames}) and settle_frames ({settle_frames}) must lie in [0, {T}): no frame to score")
    doa_max, num_period = float(doa_max), float(num_period)
    if localizer is None:
        localizer = track_localizer(beamf, bf_mat, envelope, max_batch=batch_trials)

    def path(time_vec, phase):
        return moving_doa_path(time_vec, test_duration, doa_max, num_period, phase)

    def device_batch(phase):  # moving-DoA device synthesis (micloc_synth_targets_f64, moving = 1)
        from . import synthesis

        return synthesis.apply_to_template_batch(geometry, fs, (time_test, sig_test), path(time_test, phase), device=getattr(beamf, "device", None),
                                                 device_delays=True)

    def read_out(x, _, phase):  # (errors reduced where the index is: a device tensor leaves two scalars per trial to copy)
        return track_errors(doa_list, localizer(x, time_in), path(time_in, phase), lag_frames, settle_frames)

    # the truth kept per trial is its phase (the record's `doa`); the record's `index` stays zero, `pmax` is the mean error
    phase, full, extra = _monte_carlo(
        "moving-noisy", geometry, fs, doa_list, time_test, sig_test, snr_trial, seed, mode, rank, world_size, group, batch_trials, out_dir,
        key=dict(doa_max=doa_max, num_period=num_period, lag_frames=lag_frames, settle_frames=settle_frames, win_fall=int(envelope.win_lens[0]),
                 win_rise=int(envelope.win_lens[1]), **_localizer_key(beamf, bf_mat, store_key)),
        rec=[("trial", "<i8"), ("doa", "<f8"), ("index", "<i8"), ("pmax", "<f8"), ("med", "<f8")],
        fields=(("err", "pmax", np.float64, (), 0.0), ("med", "med", np.float64, (), 0.0)), draw=_one_doa,
        host_trial=_with_noise(lambda ph: synthesize_array_signal(geometry, fs, time_test, sig_test, path(time_test, ph))),
        device_batch=device_batch, read_out=read_out)
    shape = (len(snr_db_vec), num_sim)
    e, m = full["err"].reshape(shape), full["med"].reshape(shape)
    res = dict(phase=phase.reshape(shape), err=e, med=m, track_mae_deg=np.mean(e, axis=1) * 180 / np.pi,
               track_median_deg=np.median(m, axis=1) * 180 / np.pi, lag_frames=lag_frames, settle_frames=settle_frames, snr_db_vec=snr_db_vec,
               **extra)
    res["mae_deg"] = res["track_mae_deg"]
    return res


def xylo_track_localizer(demo, envelope, max_batch=1100):
    """track_localizer's place in moving_target_sweep(localizer=) for the Xylo chain: Demo.track_batch (encoder, integer LIF, envelope
    and arg-max per frame in one read-out of the LIF walk); index [B, T] stays on the device."""

    def run(sig_batch, time_vec):
        return _in_batches(sig_batch, max_batch, lambda x: (demo.track_batch(x, envelope)["index"],))[0]

    return run


def xylo_stream_track_localizer(demo, envelope, tile, max_batch=1100):
    """stream_track_localizer's twin for the Xylo chain, for xylo_moving_target_sweep(localizer=): every batch is pushed in tiles of `tile`
    frames (multiples of 16) through a tracked Xylo stream (demo.streaming_localizer(track=envelope)) and the index [B, T] of finish()
    comes back -- the bits of Demo.track_batch on the whole batch, with np.roll's wrap-around rows known here because the batch is
    complete.  PARITY UNPINNED for the integer-LIF stage."""
    tile = int(tile)
    if tile < 1:
        raise ValueError("tile must be at least 1 frame")
    half = len(demo.beamfs[0].kernel) // 2

    def run(sig_batch, time_vec):
        def one(x):
            B, T, _ = x.shape
            s = demo.streaming_localizer(batch=B, total_frames=T, wrap_tail=_wrap_rows(x, half), max_tile=min(tile, T), track=envelope)
            for t in range(0, T, tile):
                s.push(x[:, t : t + tile, :])
            return (s.finish()["track_index"],)

        return _in_batches(sig_batch, max_batch, one)[0]

    return run


def xylo_moving_target_sweep(demo, envelope, localizer=None, batch_trials=1100, store_key=None, **kw):
    """moving_target_sweep for the Xylo chain (paper_plots/target_xylo_localization.py:672-789, `test_moving_target`, and its
    `_unipolar` twin): the same moving test signal, SNR grid and scoring, the estimate of frame t read from the hidden layer's spikes,
    `np.argmax(Envelope.evolve(spikes_out), axis=1)`.  `demo` is a xylo_snn_localization.Demo with one band; its beamformer and bf_mat
    give the geometry, the lag and the store key, which also covers the quantised specification and `bipolar`.  PARITY UNPINNED for
    the integer-LIF stage, as xylo_target_sweep.  `localizer`: e.g. the tracked stream (xylo_stream_track_localizer).  Other keywords as
    moving_target_sweep."""
    if len(demo.beamfs) != 1:
        raise ValueError(f"xylo_moving_target_sweep takes a demo with one band ({len(demo.beamfs)} given)")
    if localizer is None:
        localizer = xylo_track_localizer(demo, envelope, max_batch=batch_trials)
    key = _xylo_store_key(demo, store_key)
    res = moving_target_sweep(demo.beamfs[0], demo.bf_mats[0], demo.doa_list, envelope, localizer=localizer, batch_trials=batch_trials,
                              store_key=key, **kw)
    res["parity"] = "unpinned (integer LIF)"
    return res


def wideband_track_localizer(loc, envelope, max_batch=1100):
    """track_localizer's place in moving_target_sweep(localizer=) for a wideband localizer (wideband.WidebandSNNLocalizer or
    WidebandBeamformerLocalizer): its track_batch -- the filterbank, every band's chain, the bands' |y| added, envelope and arg-max per
    frame in one library call -- in device batches of at most `max_batch` trials; index [B, T] stays on the device.  The SNN bands'
    neuron kernels are built on the sweep's time axis, as track_localizer's."""

    def run(sig_batch, time_vec):
        return _in_batches(sig_batch, max_batch, lambda x: (loc.track_batch(x, envelope, time_vec=time_vec)["index"],))[0]

    return run


def wideband_stream_track_localizer(loc, envelope, tile, max_batch=1100):
    """stream_track_localizer's twin for a wideband localizer in wideband_moving_target_sweep(localizer=): every batch is pushed in tiles of
    `tile` frames through the tracked wideband stream (streaming.WidebandStreamingLocalizer / WidebandComplexStreamingLocalizer with
    track=envelope; SNN bands take multiples of 16) and the index [B, T] of finish() comes back -- the bits of loc.track_batch on the whole
    batch, which the wrap-around rows of every band's filtered batch (known here: the batch is complete), total_frames and the sweep's
    time axis of the neuron kernels make possible."""
    from . import runtime
    from .streaming import WidebandComplexStreamingLocalizer, WidebandStreamingLocalizer

    tile = int(tile)
    if tile < 1:
        raise ValueError("tile must be at least 1 frame")
    snn = hasattr(loc.beamfs[0], "tau_vec")
    half = len(loc.beamfs[0].kernel) // 2

    def run(sig_batch, time_vec):
        def one(x):
            import torch

            B, T, _ = x.shape
            xf = runtime.filterbank(loc.filterbank.ba_list, x, device=getattr(loc.beamfs[0], "device", None))  # [F, B, T, M]
            tail = torch.stack([_wrap_rows(xf[f], half) for f in range(xf.shape[0])])
            if snn:
                s = WidebandStreamingLocalizer(loc, B, total_frames=T, wrap_tail=tail, max_tile=min(tile, T), track=envelope, time_vec=time_vec)
            else:
                s = WidebandComplexStreamingLocalizer(loc, B, total_frames=T, wrap_tail=tail, max_tile=min(tile, T), track=envelope)
            for t in range(0, T, tile):
                s.push(x[:, t : t + tile, :])
            return (s.finish()["track_index"],)

        return _in_batches(sig_batch, max_batch, one)[0]

    return run


def wideband_moving_target_sweep(loc, envelope, localizer=None, batch_trials=1100, store_key=None, **kw):
    """moving_target_sweep read out by the WIDEBAND localizer `loc` (the form the reference deploys in its live demos) instead of one
    band: that sweep's own moving test signal, path, SNR grid, lag, settle and scoring; the estimate of frame t is the arg-max of the
    envelope of the bands' summed magnitudes (loc.track_batch).  The first band's beamformer gives the geometry, fs and the default lag;
    the store key covers the band edges, the filterbank's coefficients and every band's parameters and bf_mat hash (_wideband_store_key),
    then store_key.  `localizer`: another read-out with wideband_track_localizer's signature.  Other keywords as moving_target_sweep."""
    if localizer is None:
        localizer = wideband_track_localizer(loc, envelope, max_batch=batch_trials)
    doa_list = kw.pop("doa_list", None)
    if doa_list is None:
        doa_list = getattr(loc, "doa_list", None)
    if doa_list is None or len(doa_list) != loc.num_grid:
        raise ValueError(f"wideband_moving_target_sweep needs the localizer's DoA grid (loc.doa_list or doa_list=, {loc.num_grid} entries)")
    return moving_target_sweep(loc.beamfs[0], None, doa_list, envelope, localizer=localizer, batch_trials=batch_trials,
                               store_key={**_wideband_store_key(loc), **(store_key or {})}, **kw)


def _xylo_store_key(demo, store_key=None):
    """ShardStore key entries of a Xylo chain: the quantised specification and `bipolar`, then store_key."""
    spec = demo.spec
    return dict(chain="xylo", bipolar=bool(demo.bipolar_spikes), xylo_W_in=np.asarray(spec["W_in"]), xylo_w_rec=int(spec["w_rec"]),
                xylo_dash_syn=np.asarray(spec["dash_syn"]), xylo_dash_mem=np.asarray(spec["dash_mem"]), xylo_threshold=np.asarray(spec["threshold"]),
                **(store_key or {}))


def xylo_window_localizer(demo, window, hop, win_size, max_batch=1100):
    """device_localizer(window=)'s place in windowed_target_sweep(localizer=) for the Xylo chain: Demo.windows_batch (encoder, integer LIF
    and the read-out per window in one walk of the LIF) -> (window_peak [B, nW] int64, the window's rate at that index [B, nW])."""

    def run(sig_batch, time_vec):
        def one(x):
            out = demo.windows_batch(x, window, hop, win_size=win_size)
            a = out["window_peak"].long()
            return a.cpu().numpy(), out["window_rate"].gather(2, a.unsqueeze(2)).squeeze(2).cpu().numpy()

        return _in_batches(sig_batch, max_batch, one)

    return run


def xylo_windowed_target_sweep(demo, window, hop=None, win_size=None, localizer=None, snr_db_vec=None, num_sim=100, mode="parity",
                               test_duration=1000e-3, snr_gain_due_to_bandwidth=None, batch_trials=None, device_delays=None, store_key=None, **kw):
    """windowed_target_sweep for the Xylo chain: the trials of xylo_target_sweep (the chirp over the design band, signal_from_template,
    the same draws in both modes), every one localised per window of `window` frames every `hop` frames (multiples of 256, hop <= window)
    by find_peak_location(win_size) on the window's spike counts -- how the accuracy of the Xylo read-out depends on the pack length, the
    parameter the reference's live loop (`recording_duration`) and its snn_localization_benchmark.py (`frame_duration`) vary.  The
    network runs each trial ONCE, without a reset between windows (Demo.windows_batch).  win_size defaults to xylo_target_sweep's; the
    `window_pmax` of a window is its rate at the peak index.  With window >= T, `argmax` is xylo_target_sweep's `index`.  `demo` is a
    xylo_snn_localization.Demo with one band; the store key also covers the quantised specification, `bipolar` and win_size.
    batch_trials, device_delays: xylo_target_sweep's defaults.  PARITY UNPINNED for the integer-LIF stage, as xylo_target_sweep.
    Other keywords (seed, rank, world_size, group, out_dir) as windowed_target_sweep."""
    if len(demo.beamfs) != 1:
        raise ValueError(f"xylo_windowed_target_sweep takes a demo with one band ({len(demo.beamfs)} given)")
    window = int(window)
    hop = window if hop is None else int(hop)
    win_size = _xylo_win_size(demo.doa_list) if win_size is None else int(win_size)
    if batch_trials is None:
        batch_trials = 1100 if mode == "throughput" else 50
    if device_delays is None:
        device_delays = mode == "throughput"
    if localizer is None:
        localizer = xylo_window_localizer(demo, window, hop, win_size, max_batch=batch_trials)
    trials = _xylo_trials(demo, snr_db_vec, num_sim, test_duration, snr_gain_due_to_bandwidth, device_delays)
    key = _xylo_store_key(demo, dict(win_size=win_size, device_delays=bool(device_delays), **(store_key or {})))
    res = windowed_target_sweep(demo.beamfs[0], demo.bf_mats[0], demo.doa_list, window, hop=hop, num_sim=num_sim, mode=mode, localizer=localizer,
                                batch_trials=batch_trials, store_key=key, trials=trials, **kw)
    res["win_size"] = win_size
    res["parity"] = "unpinned (integer LIF)"
    return res


def _multi_noisy_cli(args, geometry, doa_list, fs, freq_design, freq_range, tau, rank, world):
    """--sweep multi-noisy: multi_target_sweep with the noisy sweep's SNN or complex beamformer (design as --sweep noisy) or the MUSIC
    noisy sweep's MUSIC (1 s test signal, band [0.8, 1.2] x freq_design, k = 1, N = 2048)."""
    kw = dict(num_targets=args.num_targets, min_separation=np.deg2rad(args.min_separation_deg), num_sim=args.num_sim or 100, seed=args.seed,
              mode=args.mode, rank=rank, world_size=world)
    if args.method == "music":
        from .music_beamformer import MUSIC

        music = MUSIC(geometry=geometry, freq_range=[0.8 * freq_design, 1.2 * freq_design], doa_list=doa_list, frame_duration=1.0, fs=fs)
        sep = kw["min_separation"] / 2
        loc = music_localizer(music, 1, 0.0, 2048, max_batch=100, num_sources=args.num_targets, min_separation=sep)
        return multi_target_sweep(music, None, doa_list, localizer=loc, test_duration=1000e-3, batch_trials=100,
                                  snr_gain_due_to_bandwidth=(fs / 2) / (0.4 * freq_design), store_key=_music_store_key(music, 1, 0.0, 2048), **kw)
    time_temp = np.arange(0, 1.0, step=1 / fs)
    period = time_temp[-1]
    freq_inst = freq_range[0] + (freq_range[1] - freq_range[0]) * (time_temp % period) / period
    sig_temp = np.sin(2 * np.pi * np.cumsum(freq_inst) / fs)
    if args.method == "snn":
        from .snn_beamformer import SNNBeamformer

        beamf = SNNBeamformer(geometry, kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]), freq_range=freq_range, fs=fs, bipolar_spikes=True)
        design = lambda doas: beamf.design_from_template((time_temp, sig_temp), doas, svd=args.svd)  # noqa: E731
    else:
        from .beamformer import Beamformer

        beamf = Beamformer(geometry, kernel_duration=10.0e-3, freq_range=freq_range, fs=fs)
        # (complex columns: designed whole on every rank)
        design = None
    if design is not None:
        bf_mat = sharded_design(design, doa_list, rank, world)
    else:
        bf_mat, _ = beamf.design_from_template((time_temp, sig_temp), doa_list, svd=args.svd)  # (bf_mat, cov_mat_list)
    if getattr(args, "stream_tile", None):  # the same sweep read out by the multi-source stream, tile by tile (the same bits)
        kw["localizer"] = stream_multi_localizer(beamf, bf_mat, doa_list, args.stream_tile, args.num_targets, min_separation=kw["min_separation"] / 2)
    return multi_target_sweep(beamf, bf_mat, doa_list, **kw)


def main(argv=None):
    """`python -m haghighatshoarmuir2024_amd.sweep [--sweep noisy|speech|xylo|music-noisy|music-speech|multi-noisy|windowed-noisy|moving-noisy|wideband-speech|moving-wideband]`: the accuracy sweeps of the paper scripts
    (paper_plots/target_snn_localization.py:309-520 noisy target, :97-300 speech target; target_xylo_localization.py:540-608),
    design + 11 SNRs x num_sim trials, printing what the scripts print (SNR vector and mean absolute errors in degrees)."""
    import argparse

    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--sweep", choices=["noisy", "speech", "xylo", "music-noisy", "music-speech", "multi-noisy", "windowed-noisy", "moving-noisy", "wideband-speech", "moving-wideband"],
                    default="noisy")
    ap.add_argument("--bands", type=parse_bands, default=parse_bands("1000:1600,1600:2400,2400:3400"),
                    help="wideband-speech, moving-wideband: the bands as low:high pairs in Hz, comma separated (at most 16)")
    ap.add_argument("--window-frames", type=int, default=None, help="windowed-noisy: frames per window (a multiple of the plan's window quantum; --method xylo: of 256)")
    ap.add_argument("--hop-frames", type=int, default=None, help="windowed-noisy: frames between window starts (default: --window-frames)")
    ap.add_argument("--method", choices=["snn", "beamformer", "music", "xylo"], default="snn",
                    help="multi-noisy, wideband-speech and moving-wideband (snn | beamformer), moving-noisy and windowed-noisy (snn | beamformer | xylo): the localizer")
    ap.add_argument("--num-targets", type=int, default=2, help="multi-noisy: simultaneous targets (1 .. 4)")
    ap.add_argument("--min-separation-deg", type=float, default=45.0, help="multi-noisy: least pi-periodic distance between targets")
    ap.add_argument("--stream-tile", type=int, default=None,
                    help="multi-noisy with --method snn | beamformer: read the trials out by the multi-source stream in tiles of N frames (snn: a multiple of 16)")
    ap.add_argument("--num-sim", type=int, default=None, help="trials per SNR (scripts: 100 noisy / xylo, 20 speech)")
    ap.add_argument("--grid", type=int, default=None, help="DoA grid (default: 449; music-noisy: 57, the MUSIC script's)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mode", choices=["parity", "throughput"], default="parity")
    ap.add_argument("--flac", default=None, help="speech sweep: the LibriSpeech utterance (84-121123-0020.flac of the reference's paper_plots/)")
    ap.add_argument("--pcm-npz", default=None, help="speech sweep: an .npz with `pcm16` and `rate` instead of the FLAC file")
    ap.add_argument("--svd", choices=["host", "device"], default="host", help="design_from_template decompositions")
    args = ap.parse_args(argv)

    from .array_geometry import CenterCircularArray
    from .snn_beamformer import SNNBeamformer

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group("nccl")
    fs, freq_design = 48_000, 2000.0
    freq_range = [0.5 * freq_design, freq_design]
    tau = 1.0 / (2 * np.pi * freq_design)
    geometry = CenterCircularArray(radius=4.5e-2, num_mic=7)
    music_grid = args.sweep == "music-noisy" or (args.sweep == "multi-noisy" and args.method == "music")
    grid = args.grid if args.grid is not None else (8 * 7 + 1 if music_grid else 64 * 7 + 1)
    doa_list = np.linspace(-np.pi, np.pi, grid)
    if args.method == "xylo" and args.sweep not in ("moving-noisy", "windowed-noisy"):
        ap.error("--method xylo goes with --sweep moving-noisy or windowed-noisy (the Xylo accuracy sweep is --sweep xylo)")
    if args.stream_tile is not None and (args.sweep != "multi-noisy" or args.method not in ("snn", "beamformer") or args.stream_tile < 1):
        ap.error("--stream-tile N (at least 1 frame) goes with --sweep multi-noisy --method snn or beamformer")
    if args.sweep == "windowed-noisy" and args.method == "xylo":
        from .xylo_snn_localization import Demo

        if args.window_frames is None:
            ap.error("--sweep windowed-noisy needs --window-frames")
        demo = Demo(geometry=geometry, freq_bands=[freq_range], doa_list=doa_list, recording_duration=0.25, bipolar_spikes=True, fs=fs)
        res = xylo_windowed_target_sweep(demo, args.window_frames, hop=args.hop_frames, num_sim=args.num_sim or 100, seed=args.seed, mode=args.mode,
                                         rank=rank, world_size=world)
    elif args.sweep == "moving-noisy" and args.method == "xylo":
        from .utils import Envelope
        from .xylo_snn_localization import Demo

        demo = Demo(geometry=geometry, freq_bands=[freq_range], doa_list=doa_list, recording_duration=0.25, bipolar_spikes=True, fs=fs)
        res = xylo_moving_target_sweep(demo, Envelope(rise_time=1e-3, fall_time=10e-3, fs=fs), num_sim=args.num_sim or 100, seed=args.seed,
                                       mode=args.mode, rank=rank, world_size=world)
    elif args.sweep == "moving-noisy" and args.method == "beamformer":
        from .beamformer import Beamformer
        from .utils import Envelope

        beamf = Beamformer(geometry, kernel_duration=10.0e-3, freq_range=freq_range, fs=fs)
        time_temp = np.arange(0, 1.0, step=1 / fs)
        freq_inst = freq_range[0] + (freq_range[1] - freq_range[0]) * (time_temp % time_temp[-1]) / time_temp[-1]
        bf_mat, _ = beamf.design_from_template((time_temp, np.sin(2 * np.pi * np.cumsum(freq_inst) / fs)), doa_list, svd=args.svd)
        # (a 0.1 s trial: the script's 10 ms / 100 ms envelope would still be settling at its end)
        res = moving_target_sweep(beamf, bf_mat, doa_list, Envelope(rise_time=1e-3, fall_time=10e-3, fs=fs), num_sim=args.num_sim or 100,
                                  seed=args.seed, mode=args.mode, rank=rank, world_size=world)
    elif args.sweep == "multi-noisy":
        res = _multi_noisy_cli(args, geometry, doa_list, fs, freq_design, freq_range, tau, rank, world)
    elif args.sweep == "wideband-speech":
        from .wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

        if args.method == "music":
            ap.error("--sweep wideband-speech takes --method snn or beamformer")

        if args.pcm_npz:
            z = np.load(args.pcm_npz)
            src = speech_source(fs, pcm16=z["pcm16"], rate=int(z["rate"]))
        elif args.flac:
            src = speech_source(fs, flac_path=args.flac)
        else:
            ap.error("--sweep wideband-speech needs --flac or --pcm-npz")
        # the live demo's set-up per band (micloc/localization_demo_snn.py:40-93): 0.25 s design sines, 10 ms Hilbert kernel, bipolar
        if args.method == "beamformer":  # (micloc/localization_demo.py:43-89: complex Beamformers behind the order-2 filterbank)
            loc = WidebandBeamformerLocalizer.from_bands(geometry, args.bands, doa_list, recording_duration=0.25, kernel_duration=10.0e-3, fs=fs)
        else:
            loc = WidebandSNNLocalizer.from_bands(geometry, args.bands, doa_list, recording_duration=0.25, kernel_duration=10.0e-3,
                                                  bipolar_spikes=True, fs=fs)
        res = wideband_speech_sweep(loc, doa_list, src, num_sim=args.num_sim or 20, seed=args.seed, mode=args.mode, rank=rank, world_size=world)
    elif args.sweep == "moving-wideband":
        from .utils import Envelope
        from .wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

        if args.method not in ("snn", "beamformer"):
            ap.error("--sweep moving-wideband takes --method snn or beamformer")
        # the live demos' set-up per band, as --sweep wideband-speech; the moving target and the envelope of --sweep moving-noisy
        if args.method == "beamformer":
            loc = WidebandBeamformerLocalizer.from_bands(geometry, args.bands, doa_list, recording_duration=0.25, kernel_duration=10.0e-3, fs=fs)
        else:
            loc = WidebandSNNLocalizer.from_bands(geometry, args.bands, doa_list, recording_duration=0.25, kernel_duration=10.0e-3,
                                                  bipolar_spikes=True, fs=fs)
        res = wideband_moving_target_sweep(loc, Envelope(rise_time=1e-3, fall_time=10e-3, fs=fs), num_sim=args.num_sim or 100, seed=args.seed,
                                           mode=args.mode, rank=rank, world_size=world)
    elif args.sweep.startswith("music"):
        # paper_plots/target_localization_MUSIC.py: band [0.8, 1.2] x 2 kHz, frame_duration 1.0, k = 1, N = 2048
        from .music_beamformer import MUSIC

        music = MUSIC(geometry=geometry, freq_range=[0.8 * freq_design, 1.2 * freq_design], doa_list=doa_list, frame_duration=1.0, fs=fs)
        if args.sweep == "music-speech":
            if args.pcm_npz:
                z = np.load(args.pcm_npz)
                src = speech_source(fs, pcm16=z["pcm16"], rate=int(z["rate"]))
            elif args.flac:
                src = speech_source(fs, flac_path=args.flac)
            else:
                ap.error("--sweep music-speech needs --flac or --pcm-npz")
            res = music_speech_sweep(music, src, num_sim=args.num_sim or 100, seed=args.seed, mode=args.mode, rank=rank, world_size=world)
        else:
            res = music_noisy_sweep(music, num_sim=args.num_sim or 100, seed=args.seed, mode=args.mode, rank=rank, world_size=world)
    elif args.sweep == "xylo":
        from .xylo_snn_localization import Demo

        demo = Demo(geometry=geometry, freq_bands=[freq_range], doa_list=doa_list, recording_duration=0.25, bipolar_spikes=True, fs=fs)
        res = xylo_target_sweep(demo, num_sim=args.num_sim or 100, seed=args.seed, mode=args.mode, rank=rank, world_size=world)
    else:
        beamf = SNNBeamformer(geometry, kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]), freq_range=freq_range, fs=fs, bipolar_spikes=True)
        time_temp = np.arange(0, 1.0, step=1 / fs)
        period = time_temp[-1]
        freq_inst = freq_range[0] + (freq_range[1] - freq_range[0]) * (time_temp % period) / period
        sig_temp = np.sin(2 * np.pi * np.cumsum(freq_inst) / fs)
        # the design is sharded over the DoA grid as well (one all-gather of the columns)
        bf_mat = sharded_design(lambda doas: beamf.design_from_template((time_temp, sig_temp), doas, svd=args.svd), doa_list, rank, world)
        if args.sweep == "speech":
            if args.pcm_npz:
                z = np.load(args.pcm_npz)
                src = speech_source(fs, pcm16=z["pcm16"], rate=int(z["rate"]))
            elif args.flac:
                src = speech_source(fs, flac_path=args.flac)
            else:
                ap.error("--sweep speech needs --flac or --pcm-npz")
            res = speech_target_sweep(beamf, bf_mat, doa_list, src, num_sim=args.num_sim or 20, seed=args.seed, mode=args.mode, rank=rank, world_size=world)
        elif args.sweep == "moving-noisy":
            if args.method != "snn":
                ap.error("--sweep moving-noisy takes --method snn, beamformer or xylo")
            from .utils import Envelope

            # (a 0.1 s trial: the script's 10 ms / 100 ms envelope would still be settling at its end)
            res = moving_target_sweep(beamf, bf_mat, doa_list, Envelope(rise_time=1e-3, fall_time=10e-3, fs=fs), num_sim=args.num_sim or 100,
                                      seed=args.seed, mode=args.mode, rank=rank, world_size=world)
        elif args.sweep == "windowed-noisy":
            if args.window_frames is None:
                ap.error("--sweep windowed-noisy needs --window-frames")
            res = windowed_target_sweep(beamf, bf_mat, doa_list, args.window_frames, hop=args.hop_frames, num_sim=args.num_sim or 100, seed=args.seed,
                                        mode=args.mode, rank=rank, world_size=world)
        else:
            res = noisy_target_sweep(beamf, bf_mat, doa_list, num_sim=args.num_sim or 100, seed=args.seed, mode=args.mode, rank=rank, world_size=world)
    if rank == 0:
        print(f"SNR: {res['snr_db_vec']}")
        print(f"Mean aboslute errors: {res['mae_deg']}")
        if "resolved_rate" in res:
            print(f"Resolution rate: {res['resolved_rate']}")
        if "track_median_deg" in res:
            print(f"Median tracking errors: {res['track_median_deg']}")
        if "window_mae_deg" in res:
            print(f"Window starts (frames): {res['window_start']}")
            print(f"Mean aboslute errors per window:\n{res['window_mae_deg']}")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
