#!/usr/bin/env python3
"""Headline benchmark: audio frames/s through the full STHT -> RZCC -> SNN-beamform pipeline.

Default workload (BASELINE.json configs[1], target_snn_localization.py): 7-mic centre-circular array, 48 kHz,
0.1 s noisy 2 kHz test tone (T = 4799 frames), 11 SNRs x 100 Monte-Carlo trials = 1100 trials per step,
DoA grid 360 (BASELINE's nominal grid; `--grid 449` selects the script-exact one), bf_mat designed from the
1 s 1->2 kHz chirp with design_from_template on the device before timing.  One "step" = one pass of the
hot path over the 1100-trial batch (inputs resident in HBM): STHT, band-pass, RZCC, LIF, beamforming,
power, arg-max, DoA error / MAE.  Weak scaling: every rank processes its own 1100-trial batch.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--grid G] [--config noisy|speech|stress|xylo] [--dump-outputs DIR] [--full]

A plain run sets up (ending with `--settle-seconds` of headline steps), warms up, times ONE region of exactly K steps, optionally
writes the last step's outputs (`--dump-outputs`) and prints the line: `value` / `ms_per_step` and what is known without further runs.  `--full` adds everything else this file
measures: five timed regions (median), the sustained region with clock / power telemetry, the end-to-end and variant clocks, the
per-kernel stage times and roofline (with live rocprofv3 traffic passes), the CPU baselines, the reference-MAE / per-call /
complex-beamformer / streaming blocks and the other workloads as child runs.

`--gpus N` (N > 1) without a launcher: this process stays GPU-free and starts N ranks of itself (one per GPU,
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, RCCL process group); under `python -m torch.distributed.run`
(WORLD_SIZE already set) it is one of the ranks.  Rank 0 prints ONE JSON line (DESIGN.md "Measurement").

Other workloads (same JSON contract, their own `config.workload`, not the headline):
  --config speech   BASELINE configs[2], per-GPU share: 125 trials of the LibriSpeech utterance (T = 332 157)
  --config stress   BASELINE configs[4], 64 mics / 96 kHz / 1440 DoAs, `--trials` trials per GPU (default 256)
  --config xylo     BASELINE configs[3], target_xylo_localization.py: 1 s chirp (T = 48 000), order-1 band-pass, bipolar RZCC,
                    integer LIF hidden layer (one neuron per DoA), find_peak_location -- PARITY UNPINNED for the LIF stage

`value` times the hot path on a batch resident in HBM (the driver's contract); `value_e2e` (--full) adds everything in front of
it inside the same captured graph: DoA draw, array-signal synthesis and AWGN on the device, fresh numbers every step.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# stage key in `stages_ms` -> device symbol that dominates it (what rocprofv3 lists)
KERNEL_SYMBOL = {"beamform_kernel": "beamform_ws_kernel", "stht_kernel": "stht_kernel", "bandpass_rzcc_kernel": "bandpass_rzcc"}
FP64_MFMA_PEAK_TFLOPS = 78.6  # MI355X datasheet fp64 matrix = fp64 vector = 1/2 of the 157.3 TF fp32 rate in MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=["noisy", "speech", "stress", "xylo"], default="noisy")
    ap.add_argument("--grid", type=int, default=None, help="DoA grid size (default: 360; stress: 1440)")
    ap.add_argument("--trials", type=int, default=None, help="trials per rank per step (default: 1100 = 11 SNRs x 100; speech 125; stress 256)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU time of each cpu_baseline leg")
    ap.add_argument("--full", action="store_true", help="everything besides the headline figure: see the module docstring (off by default)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed in its last step (rank 0) as "
                    "DIR/<name>.npy, float64, at most 64 MB in all")
    ap.add_argument("--settle-seconds", type=float, default=0.25, help="end the set-up with about this long of headline steps before the "
                    "--warmup steps, so that a short timed region does not start while clock and power management settle; 0: none "
                    "(the timed region follows the warm-up steps cold); the count is reported as config.settle_steps")
    ap.add_argument("--repeats", type=int, default=None, help="the K-step timed region is run this many times; ms_per_step / value are the median "
                    "(default 1; 5 with --full)")
    ap.add_argument("--no-other-configs", action="store_true", help="--full: skip the speech / xylo / stress child runs and the reference-MAE / per-call blocks")
    ap.add_argument("--streams", type=int, default=None, help="HIP streams consecutive steps are pipelined over (1 = serial; default 3, "
                    "4 with the scan-lane schedule)")
    ap.add_argument("--schedule", choices=["auto", "graphs", "scan-lane"], default="auto", help="graphs: one captured hipGraph per stream, replayed "
                    "round-robin.  scan-lane: eager launches, the serial checkpoint scans of all batches on one stream that owns --scan-lane-cus "
                    "compute units of every XCD, everything else on streams restricted to the other units (runtime.StreamPipeline).  auto: scan-lane "
                    "for the speech workload (long recordings: the scan is a 10 ms latency chain on 28 workgroups), graphs otherwise")
    ap.add_argument("--scan-lane-cus", type=int, default=4, help="compute units per XCD of the scan lane")
    ap.add_argument("--xylo-lif", default="static", help="xylo: 'static' (one workgroup per trial: what the three-stream step runs best with) or "
                    "'queue' / 'queue:<workgroups per CU>' (persistent workgroups on the ticket queue: the faster launch when it runs alone)")
    ap.add_argument("--cpu-cores", type=int, default=None, help="pin every rank to this many host cores (its own slice of the allowed set) before "
                    "anything touches the GPU: 2 = a rank's share of a 16-core cgroup at 8 ranks")
    ap.add_argument("--baseline-total", action="store_true", help="speech / stress: split BASELINE's sweep totals (1000 / 16384 trials) over the "
                    "ranks (strong scaling: total work fixed) instead of a fixed batch per rank")
    ap.add_argument("--encoder-chunk", type=int, default=None, help="frames per time chunk of the band-pass / RZCC stage (default: the library's automatic choice; < 0: never chunk)")
    ap.add_argument("--traffic-bytes", type=float, default=None, help="override roofline.traffic (HBM bytes per dominant-kernel launch)")
    ap.add_argument("--sustained-seconds", type=float, default=None, help="length of the `sustained` region (one long run of headline steps with the "
                    "shader clock / socket power sampled in-process); 0 disables it (default 0; 5 with --full)")
    ap.add_argument("--other-sustained-seconds", type=float, default=10.0, help="length of the sustained region of each `other_configs` child run "
                    "(speech / xylo / stress: their steady-state ms per step with clock and power telemetry); 0 disables it")
    ap.add_argument("--no-live-traffic", action="store_true", help="do not measure roofline.traffic in a rocprofv3 child of this run; read the "
                    "committed profile instead (only if its MANIFEST says it was taken on the current csrc/beamform.hip)")
    ap.add_argument("--share-device", action="store_true", help="REHEARSAL of the N > 1 launch on a box with ONE GPU: all --gpus ranks use device 0, the "
                    "process group is gloo (RCCL refuses two ranks on one device) and every collective is staged through host memory; everything "
                    "else -- the rank launcher, per-rank batches and trial numbering, barriers, per-rank clocks, MAX reduce, the exchange step, the "
                    "MAE from the gathered trials -- is the code of the real launch.  The ranks time-slice one GPU: `value` is NOT a scaling figure")
    ap.add_argument("--as-rank", type=int, default=None, help=argparse.SUPPRESS)  # test hook: build rank R's workload in a single process (no group)
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)  # the program rocprofv3 runs for the live PMC passes
    ap.add_argument("--pmc-summary", default=None, help="committed rocprofv3 PMC summary to read roofline.traffic from (default: newest profiles/r*/pmc_summary.csv)")
    # test hook (tests/test_bench_launch_cpu.py): exercise the rank launcher and the collective code on CPU with gloo
    ap.add_argument("--cpu-stub", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if args.sustained_seconds is None:
        args.sustained_seconds = 5.0 if args.full else 0.0
    if args.schedule == "auto":
        args.schedule = "scan-lane" if args.config == "speech" else "graphs"
    args.streams_given = args.streams is not None
    if args.streams is None:
        args.streams = 4 if args.schedule == "scan-lane" else 3
    return args


# ----------------------------------------------------------------------------------------------------------------
# rank launcher (runs in a process that has not touched the GPU)
# ----------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def visible_gpus():
    import torch

    return int(torch.cuda.device_count())  # counts devices without initialising the HIP runtime state of this process


def launch_ranks(args, argv):
    """Start `args.gpus` copies of this script, one per GPU, as CHILD processes (never exec from a GPU-initialised
    process) and return the exit code of the job.  Rank 0's stdout (the JSON line) passes straight through."""
    n = args.gpus
    if not args.cpu_stub:
        have = visible_gpus()
        if args.share_device and have >= 1:
            have = n  # rehearsal: every rank on device 0
        if have < n:
            print(f"bench.py: --gpus {n} requested but only {have} HIP device(s) visible", file=sys.stderr)
            return 2
    env0 = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n))
    procs = []
    for r in range(n):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    alive = set(range(n))
    while alive:
        for r in list(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and rc == 0:
                rc = code
                for o in alive:  # one rank failed: the others would wait in a collective for ever
                    procs[o].terminate()
        time.sleep(0.05)
    return rc


# ----------------------------------------------------------------------------------------------------------------
# workloads
# ----------------------------------------------------------------------------------------------------------------
def chirp_template(fs, freq_range):
    # target_snn_localization.py:345-356
    time_temp = np.arange(0, 1.0, step=1 / fs)
    period = time_temp[-1]
    freq_inst = freq_range[0] + (freq_range[1] - freq_range[0]) * (time_temp % period) / period
    return time_temp, np.sin(2 * np.pi * np.cumsum(freq_inst) / fs)


def speech_source(fs):
    """The LibriSpeech utterance of BASELINE config 3 (84-121123-0020.flac, decoded by haghighatshoarmuir2024_amd.flac and
    kept as PCM in tests/golden/speech_trial.npz), resampled like target_snn_localization.py:149-154."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "speech_trial.npz"))
    rate = int(z["rate"])
    sig = z["pcm16"].astype(np.float64) / 32768.0
    t = np.arange(len(sig)) / rate
    t_fs = np.linspace(t[0], t[-1], int(len(sig) / rate * fs))
    return t_fs, np.interp(t_fs, t, sig)


def build_workload(args, rank, device):
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray, Random2DArray
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer, neuron_impulse_response

    cfg = args.config
    t_design = None
    freq_design = 2000.0
    freq_range = [0.5 * freq_design, freq_design]
    tau = 1.0 / (2 * np.pi * freq_design)
    if cfg == "stress":
        fs, num_mic = 96_000, 64
        np.random.seed(1)  # Random2DArray draws from the global NumPy stream (array_geometry.py:126-127)
        geometry = Random2DArray(radius=0.2, num_mic=num_mic)
        G = args.grid or 1440
        B = args.trials or (-(-16384 // max(1, args.world)) if args.baseline_total else 256)
    else:
        fs, num_mic = 48_000, 7
        geometry = CenterCircularArray(radius=4.5e-2, num_mic=num_mic)
        G = args.grid or 360
        B = args.trials or ((-(-1000 // max(1, args.world)) if args.baseline_total else 125) if cfg == "speech" else 1100)
    beamf = SNNBeamformer(geometry=geometry, kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]), freq_range=freq_range, fs=fs,
                          bipolar_spikes=True, device=device)
    doa_list = np.linspace(-np.pi, np.pi, G)
    # the whole design on the device: delayed templates, chain, membrane covariance (lif_cov_kernel / lif_cov_wide_kernel), batched
    # Jacobi decompositions (micloc_design_vectors_f64: two-sided up to 16 microphones, one-sided up to 64 -- config 5's 128 x 128
    # matrices); a one-off cost outside the timed region
    kw = dict(svd="device", doa_batch=240) if cfg == "stress" else dict(svd="device")
    # warm-up with one full chain batch: module load and the workspace's allocation (tens of GB at config 5) are not the design
    beamf.design_from_template(chirp_template(fs, freq_range), doa_list[: kw.get("doa_batch", 32)], **kw)
    torch.cuda.synchronize()
    t_design = time.perf_counter()
    bf_mat = beamf.design_from_template(chirp_template(fs, freq_range), doa_list, **kw)
    torch.cuda.synchronize()
    t_design = time.perf_counter() - t_design

    # test signals (target_snn_localization.py:435-455 / :148-154,213-245): synthetic, generated here, noise drawn on the device
    if cfg == "speech":
        time_test, sig_test = speech_source(fs)
        snr_gain = 1.0  # the speech sweep applies no bandwidth correction (target_snn_localization.py:227)
    else:
        time_test = np.arange(0, 100e-3, step=1 / fs)
        sig_test = np.sin(2 * np.pi * freq_design * time_test)
        snr_gain = (fs / 2) / (freq_range[1] - freq_range[0])
    snr_db_vec = np.linspace(-10, 20, 11)
    groups = len(snr_db_vec) if B % len(snr_db_vec) == 0 else 1
    snr_db = snr_db_vec[(np.arange(B) * len(snr_db_vec)) // B] - 10 * np.log10(snr_gain)
    from haghighatshoarmuir2024_amd import synthesis

    def make_batch(i):
        """Batch i of this rank: its own DoAs and its own noise (Philox substream i; trials numbered globally) -- consecutive
        steps of the timed loop are INDEPENDENT batches, one resident input tensor per HIP stream."""
        rng = np.random.RandomState(1000 + rank + 7919 * i)
        doa_i = rng.rand(B) * 2 * np.pi
        t_in, x_i = beamf.synthesize_batch((time_test, sig_test), doa_i)  # device synthesis, bit-exact with np.interp
        synthesis.add_noise_(x_i, snr_db, seed=1234, substream=i, first_trial=rank * B)  # Philox-4x32-10 + Box-Muller kernel, in place
        return t_in, x_i, doa_i

    time_in, x, doa = make_batch(0)

    plan = beamf.plan()
    nir = neuron_impulse_response(time_in[: min(len(time_in), 48_000)], beamf.tau_vec)
    plan.set_neuron_kernel(nir)
    plan.set_bf_mat(bf_mat)
    if args.encoder_chunk is not None:
        plan.set_encoder_chunk(args.encoder_chunk)
    return dict(beamf=beamf, plan=plan, x=x, doa=torch.from_numpy(doa).to(device), doa_list=torch.from_numpy(doa_list).to(device),
                bf_mat=bf_mat, nir=nir, snr_groups=groups, fs=fs, encoder_chunk=args.encoder_chunk,
                template=(time_test, sig_test), snr_db=snr_db, rank=rank, design_seconds=t_design, freq_range=freq_range,
                make_batch=make_batch)


def make_step(wl, nstreams, variants=True, scan_lane=0, e2e=True):
    # variants: True = covariance + fp32 tails (noisy workload), None = covariance only, False = none (a plain run, debugging)
    # e2e: also the end-to-end step (input side inside the graph); a plain run does not build it
    """One step = one pass of the hot path over the batch.  Consecutive steps are independent batches, so they are
    dispatched round-robin over `nstreams` HIP streams (one plan/workspace each): the latency-bound RZCC kernel of
    one step overlaps the throughput-bound STHT / beamforming kernels of its neighbours."""
    from haghighatshoarmuir2024_amd import runtime
    from haghighatshoarmuir2024_amd.runtime import StreamPipeline

    import torch as _torch

    x, doa, doa_list, S = wl["x"], wl["doa"], wl["doa_list"], wl["snr_groups"]
    plans = [wl["plan"]]
    # one resident batch per stream: stream 0 replays wl["x"] (the batch the CPU baseline and the stage timers see), the others their
    # own trials -- three readers of ONE tensor would share L2 / Infinity-Cache hits a real sweep does not get
    inputs = {id(wl["plan"]): (x, doa)}
    for i in range(1, nstreams):
        p = wl["beamf"].new_plan()
        p.set_neuron_kernel(wl["nir"])
        p.set_bf_mat(wl["bf_mat"])
        if wl.get("encoder_chunk") is not None:
            p.set_encoder_chunk(wl["encoder_chunk"])
        plans.append(p)
        _, x_i, doa_i = wl["make_batch"](i)
        inputs[id(p)] = (x_i, _torch.from_numpy(doa_i).to(x.device))
    pipe = StreamPipeline(plans, scan_lane=scan_lane)

    def body(plan, cov=False):
        xs, doas = inputs[id(plan)]
        if cov == "f32":
            out = plan.snn_pipeline_f32bf(xs)
        else:
            out = plan.snn_pipeline_cov(xs, want_power=True) if cov else plan.snn_pipeline(xs, want_power=True)
        # DoA error per trial + MAE per SNR on the device (micloc_doa_error_f64): the graph holds micloc kernels only
        _, mae = runtime.doa_error(out["argmax"], doa_list, doas, groups=S, want_err=False)
        return out, mae

    # one HIP graph per stream (pipeline kernels + the DoA-error / MAE kernel), replayed round-robin
    replay_direct = pipe.capture(lambda plan: body(plan, False)) if not scan_lane else None
    small = variants and x.shape[2] * 2 <= 64
    replay_cov = pipe.capture(lambda plan: body(plan, True)) if (variants is not False and x.shape[2] * 2 <= 128) else None
    replay_f32 = pipe.capture(lambda plan: body(plan, "f32")) if small else None

    # end-to-end variant: the whole Monte-Carlo trial on the device, per step and per stream
    #   epoch += 1 -> DoAs ~ U[0, 2 pi) -> delays.min() -> delayed-template synthesis -> AWGN at the trial's SNR -> hot path
    # (target_snn_localization.py:452-467; generators: csrc/rng.hip, synthesis: csrc/synth.hip with in-kernel delays)
    import torch

    from haghighatshoarmuir2024_amd import synthesis

    beamf = wl["beamf"]
    dev = x.device
    B, T, M = x.shape
    tpl = geo = snr_dev = None
    e2e_state = {}
    if e2e:
        t_in, s_in = synthesis._resample(*wl["template"], beamf.fs)
        tpl = runtime.Template(t_in, s_in, beamf.fs, device=dev)
        geo = runtime.Geometry(beamf.geometry, device=dev)
        snr_dev = torch.from_numpy(np.ascontiguousarray(wl["snr_db"])).to(dev)
    for i, p in enumerate(plans if e2e else []):
        e2e_state[id(p)] = dict(x=torch.empty_like(x), doa=torch.empty((B,), dtype=torch.float64, device=dev),
                                shift=torch.empty((B,), dtype=torch.float64, device=dev),
                                epoch=torch.full((1,), (wl["rank"] * 64 + i) << 20, dtype=torch.int32, device=dev),
                                ws=runtime.awgn_workspace(B, T, M, dev))

    def body_e2e(plan):
        st = e2e_state[id(plan)]
        runtime.counter_add_(st["epoch"], 1)
        runtime.uniform(B, 77, substream=0, lo=0.0, hi=2 * np.pi, out=st["doa"], epoch=st["epoch"])
        runtime.delay_min(st["doa"].view(B, 1), geo, out=st["shift"])
        # synthesis + AWGN fused: the noise-free signal is never stored (micloc_synth_awgn_f64; same bits as synth_targets + awgn_)
        runtime.synth_awgn(tpl, "apply_to_template", snr_dev, seed=77, substream=0, epoch=st["epoch"], ws=st["ws"], doa=st["doa"].view(B, 1),
                           geometry=geo, shift=st["shift"], out=st["x"])
        out = plan.snn_pipeline(st["x"], want_power=True)
        _, mae = runtime.doa_error(out["argmax"], doa_list, st["doa"], groups=S, want_err=False)
        return out, mae

    replay_e2e = pipe.capture(body_e2e) if (e2e and not scan_lane) else None

    # scan-lane schedule (long recordings): the same calls launched eagerly, the serial scan of every batch on the pipeline's lane
    # (runtime.StreamPipeline.snn_pipeline); a step is a handful of millisecond-scale launches, a graph saves nothing here
    lane_out, lane_out_e2e = [None] * len(plans), [None] * len(plans)

    def e2e_before(i):
        st = e2e_state[id(plans[i])]
        runtime.counter_add_(st["epoch"], 1)
        runtime.uniform(B, 77, substream=0, lo=0.0, hi=2 * np.pi, out=st["doa"], epoch=st["epoch"])
        runtime.delay_min(st["doa"].view(B, 1), geo, out=st["shift"])
        runtime.synth_awgn(tpl, "apply_to_template", snr_dev, seed=77, substream=0, epoch=st["epoch"], ws=st["ws"], doa=st["doa"].view(B, 1),
                           geometry=geo, shift=st["shift"], out=st["x"])

    def step_lane(cov=False, index=None):
        if cov == "e2e":
            return pipe.snn_pipeline(lambda i: e2e_state[id(plans[i])]["x"], before=e2e_before, index=index, out=lane_out_e2e, want_power=True,
                                     after=lambda i, o: runtime.doa_error(o["argmax"], doa_list, e2e_state[id(plans[i])]["doa"], groups=S, want_err=False)[1])
        if cov:
            return replay_cov(index)
        return pipe.snn_pipeline(lambda i: inputs[id(plans[i])][0], index=index, out=lane_out, want_power=True,
                                 after=lambda i, o: runtime.doa_error(o["argmax"], doa_list, inputs[id(plans[i])][1], groups=S, want_err=False)[1])

    def step(cov=False, index=None):
        # index: replay a given stream's graph (the comparisons between variants read stream 0's batch, wl["x"])
        if scan_lane:
            return step_lane(cov, index)
        if cov == "e2e":
            return replay_e2e(index)
        if cov == "f32":
            return replay_f32(index)
        return replay_cov(index) if cov else replay_direct(index)

    # every tensor a captured graph reads must outlive it: the replay closures hold the graphs and their outputs only
    step.keepalive = (e2e_state, tpl, geo, snr_dev, x, doa, doa_list, plans, inputs)
    return step, pipe


def stage_times(wl, iters):
    """Average duration of each kernel group of the FUSED pipeline (HIP events on the launch stream), in ms: exactly the
    launches one step makes (micloc_snn_pipeline_stages_f64 with one stage bit at a time, sharing one workspace)."""
    import torch

    plan, x = wl["plan"], wl["x"]
    out = plan.snn_pipeline(x, want_power=True)  # allocates the outputs, fills the workspace intermediates
    res = {}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0 = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        e1 = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        for i in range(iters):
            e0[i].record()
            for _ in range(4):  # back to back inside one bracket: the launch gap after an event is paid once, not per launch
                fn()
            e1[i].record()
        torch.cuda.synchronize()
        return float(np.mean([a.elapsed_time(b) for a, b in zip(e0, e1)])) / 4

    res["stht_kernel"] = timed(lambda: plan.snn_pipeline(x, stages=1, out=out))
    res["bandpass_rzcc_kernel"] = timed(lambda: plan.snn_pipeline(x, stages=2, out=out))
    res["beamform_kernel"] = timed(lambda: plan.snn_pipeline(x, stages=4, out=out))
    return res


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores():
    """Host cores this process may actually use: the scheduler affinity, capped by the cgroup CPU quota (a GPU box
    reports all 256 hardware threads in os.cpu_count() but grants a 16-CPU share per GPU)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(np.ceil(int(txt[0]) / int(txt[1])))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(np.ceil(q / per))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


# ---- the reference-style NumPy chain trial-parallel over the host cores (SURVEY 8d ii) -----------------------------------------
# Worker PROCESSES (one BLAS / OpenMP thread each), started by `numpy_pool()` BEFORE this process touches the GPU -- a pool forked or
# spawned from a GPU-initialised process would be the exec the pool forbids -- and idle (blocked on a pipe) until cpu_baseline feeds them.
_NP_ORACLE = None


def _np_worker_init():
    global _NP_ORACLE
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    try:
        from threadpoolctl import threadpool_limits

        threadpool_limits(1)
    except Exception:
        pass
    import scipy.signal  # noqa: F401  (snn_chain_numpy imports it on its first call: paid here, not inside the timed leg)
    from oracle import oracle as O

    _NP_ORACLE = O


def _np_worker(task):
    xs, chain_args = task
    return [int(_NP_ORACLE.snn_chain_numpy(x, *chain_args)["argmax"]) for x in xs]


def numpy_pool(workers):
    import multiprocessing as mp

    saved = {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")}
    os.environ.update({k: "1" for k in saved})  # inherited by the workers only: restored below for this process
    try:
        pool = mp.get_context("spawn").Pool(workers, initializer=_np_worker_init)
        try:
            # every worker is up and has imported NumPy / SciPy / the oracle -- or the leg is dropped (a worker that dies in its
            # initialiser is respawned for ever: never wait for that without a limit)
            pool.map_async(_np_worker, [([], ())] * workers).get(timeout=180)
        except Exception:
            pool.terminate()
            raise
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return pool


def cpu_baseline(wl, budget_s, pool=None, pool_workers=0):
    """The CPU restatement of the same hot path on the first trials of the SAME batch, three ways:
      value            the C oracle, trial-parallel over all host cores (one thread per core)
      single_thread    the C oracle on one core
      numpy_ops        the reference's own op sequence (NumPy / SciPy calls, BLAS threads at their default), one process
      numpy_ops_all_cores   the same op sequence trial-parallel over `pool_workers` worker processes, one BLAS thread each -- north_star's
                            "reference NumPy CPU path timed on the same box's host cores" (the pool was started before any GPU call)
    Each leg is sized for about `budget_s` seconds from a short calibration run."""
    from oracle import oracle as O

    beamf = wl["beamf"]
    b, a = beamf.bandpass_filter
    w = beamf.spk_encoder.robust_width
    B, T, M = wl["x"].shape
    G = wl["bf_mat"].shape[1]
    host_cpus = os.cpu_count() or 1
    cores = usable_cores()
    O.lib()
    args = (beamf.kernel, b, a, w, True, wl["nir"], wl["bf_mat"])

    def sized(rate, cap):
        return int(max(1, min(cap, rate * budget_s)))

    x_cal = wl["x"][: min(B, 4)].cpu().numpy()
    t0 = time.perf_counter()
    O.snn_chain_batch(x_cal, *args)
    per_trial = (time.perf_counter() - t0) / len(x_cal)

    n1 = sized(1.0 / per_trial, B)
    x1 = wl["x"][:n1].cpu().numpy()
    t0 = time.perf_counter()
    _, am1 = O.snn_chain_batch(x1, *args)
    dt1 = time.perf_counter() - t0

    xa = wl["x"].cpu().numpy()
    ncal = min(B, 4 * cores)  # calibrate the parallel leg on a short parallel run (threads rarely scale linearly)
    t0 = time.perf_counter()
    O.snn_chain_batch_parallel(xa[:ncal], *args, threads=cores)
    par_rate = ncal / (time.perf_counter() - t0)
    reps = max(1, int(round(sized(par_rate, 64 * B) / B)))  # the whole batch, repeated if the box has many cores
    t0 = time.perf_counter()
    for _ in range(reps):
        _, am_all = O.snn_chain_batch_parallel(xa, *args, threads=cores)
    dta = time.perf_counter() - t0

    t0 = time.perf_counter()
    r0 = O.snn_chain_numpy(xa[0], *args)
    per_np = time.perf_counter() - t0
    nn = sized(1.0 / per_np, min(B, 400))
    t0 = time.perf_counter()
    am_np = [O.snn_chain_numpy(xa[i], *args)["argmax"] for i in range(nn)]
    dtn = time.perf_counter() - t0
    del r0

    np_all = None
    am_pool = None
    if pool is not None:
        # tasks of 2 trials each; sized from the one-process rate (processes rarely scale linearly: the leg reports what it measured)
        n_all = sized(pool_workers / (dtn / nn), 64 * B)
        passes = max(1, n_all // B)  # the whole batch, repeated if the box has many cores (like the C leg)
        n_all = B if passes > 1 else (max(2 * pool_workers, n_all - n_all % 2) if B >= 2 * pool_workers else B)
        tasks = [(xa[i : i + 2], args) for _ in range(passes) for i in range(0, n_all, 2)]
        t0 = time.perf_counter()
        parts = pool.map_async(_np_worker, tasks, chunksize=1).get(timeout=max(120.0, 20.0 * budget_s))
        dtp = time.perf_counter() - t0
        am_pool = np.asarray([v for p_ in parts for v in p_])
        done_trials = len(am_pool)
        am_pool = am_pool[:n_all]  # (every pass gives the same arg-max: the comparison needs one)
        np_all = dict(value=done_trials * T / dtp, unit="frames/s", cores=pool_workers,
                      sample=f"{passes} x the first {n_all} trials, {dtp:.1f} s, oracle.snn_chain_numpy (the reference's NumPy/SciPy op sequence) in "
                             f"{pool_workers} worker processes, one BLAS thread each, trials handed out two at a time; speed-up over the one-process leg "
                             f"(BLAS threads at their default) {(done_trials / dtp) / (nn / dtn):.1f}x")

    shape = f"T={T}, M={M}, G={G}"
    legs = dict(all=am_all, one=am1, numpy=np.asarray(am_np))
    if am_pool is not None:
        legs["numpy_all"] = am_pool
    extra = dict(numpy_ops_all_cores=np_all) if np_all else {}
    return dict(**extra, value=reps * B * T / dta, unit="frames/s", cores=cores, kind="port", cpu_model=cpu_model(), host_cpus=host_cpus,
                sample=f"{reps} x all {B} trials of the same batch ({shape}), {dta:.1f} s, oracle/micloc_oracle.c, trials split over {cores} threads",
                single_thread=dict(value=n1 * T / dt1, unit="frames/s", cores=1,
                                   sample=f"first {n1} trials, {dt1:.1f} s, oracle/micloc_oracle.c, one thread"),
                numpy_ops=dict(value=nn * T / dtn, unit="frames/s", cores="BLAS default",
                               sample=f"first {nn} trials, {dtn:.1f} s, oracle.snn_chain_numpy: the reference's NumPy/SciPy op sequence, one process"),
                ), legs


def traffic_from_profiles(symbol, grid_size, path=None):
    """HBM bytes per launch of `symbol` at launch size `grid_size` (work-items) from a COMMITTED rocprofv3 PMC summary
    (tools/summarize_profiles.py pmc): 2 x FETCH_SIZE + WRITE_SIZE, both KiB, FETCH_SIZE doubled as MI355X_MICROARCH.md
    "HBM" prescribes for gfx950.  Returns (bytes or None, source)."""
    import csv
    import glob

    if path is None:
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_summary.csv")),
                       key=lambda p: int("".join(c for c in os.path.basename(os.path.dirname(p)) if c.isdigit()) or 0))
        if not cands:
            return None, None
        path = cands[-1]
    fetch = write = None
    try:
        for r in csv.DictReader(open(path)):
            if symbol in r["kernel"] and int(float(r["grid_size"])) == grid_size:
                if r["counter"] == "FETCH_SIZE":
                    fetch = float(r["mean_value"])
                elif r["counter"] == "WRITE_SIZE":
                    write = float(r["mean_value"])
    except (OSError, KeyError, ValueError):
        return None, None
    if fetch is None or write is None:
        return None, os.path.relpath(path, ROOT)
    return (2.0 * fetch + write) * 1024.0, os.path.relpath(path, ROOT)



class GpuTelemetry:
    """Shader clock, socket power and hot-spot temperature of ONE device, sampled in-process by a thread (amdsmi: readable by an
    ordinary user on the GPU box, ~0.5 ms per sample -- tools/dev/clock_sources.py).  No helper process, nothing exec'ed."""

    def __init__(self, device_index, period_s=0.05):
        import threading

        self.samples = []  # (t, sclk MHz, socket W, hotspot C)
        self.period = period_s
        self.source = None
        self._stop = threading.Event()
        self._thread = None
        try:
            import amdsmi
            import torch

            amdsmi.amdsmi_init()
            hs = amdsmi.amdsmi_get_processor_handles()
            pr = torch.cuda.get_device_properties(device_index)
            want = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            sel = [h for h in hs if str(amdsmi.amdsmi_get_gpu_device_bdf(h)).lower() == want]
            self._h = sel[0] if sel else (hs[0] if len(hs) == 1 else None)
            self._smi = amdsmi
            if self._h is not None:
                self._read()
                self.source = f"amdsmi gpu_metrics (in-process, every {int(period_s * 1e3)} ms), device {want}"
        except Exception as e:  # no amdsmi / no permission: the block says so instead of inventing numbers
            self.source = None
            self.error = f"{type(e).__name__}: {e}"[:200]

    def _read(self):
        m = self._smi.amdsmi_get_gpu_metrics_info(self._h)
        clks = [c for c in m.get("current_gfxclks", []) if isinstance(c, (int, float)) and 0 < c < 10000]
        clk = float(np.mean(clks)) if clks else float(m.get("current_gfxclk"))
        return (time.perf_counter(), clk, float(m.get("current_socket_power")), float(m.get("temperature_hotspot")),
                float(min(clks)) if clks else clk)

    def start(self):
        import threading

        if self.source is None:
            return self
        self.samples = []
        self._stop.clear()

        def loop():
            while not self._stop.is_set():
                try:
                    self.samples.append(self._read())
                except Exception:
                    pass
                self._stop.wait(self.period)

        self._thread = threading.Thread(target=loop, daemon=True)
        self._thread.start()
        return self

    def stop(self):
        if self._thread is not None:
            self._stop.set()
            self._thread.join(2.0)
            self._thread = None
        if self.source is not None:
            try:
                self._smi.amdsmi_shut_down()  # (every GpuTelemetry initialises the library itself)
            except Exception:
                pass
            self.source_was, self.source = self.source, None

    def window(self, t0, t1):
        """Mean / min of the samples taken in [t0, t1) (perf_counter times)."""
        w = [s for s in self.samples if t0 <= s[0] < t1]
        if not w:
            return None
        a = np.asarray(w)
        return {"samples": len(w), "sclk_mhz_mean": float(a[:, 1].mean()), "sclk_mhz_min_xcd": float(a[:, 4].min()),
                "socket_w_mean": float(a[:, 2].mean()), "socket_w_max": float(a[:, 2].max()), "hotspot_c_max": float(a[:, 3].max())}


def sustained_block(step, pipe, args, ms_region, frames_per_step, device_index):
    """ONE region of >= --sustained-seconds of headline steps (no barrier inside: `pipe.synchronize()` only every ~0.5 s to take a
    time stamp), against the K-step regions `value` comes from: ms per step over the whole region, over its first and its last
    second, and the shader clock / socket power / hot-spot temperature the device reported meanwhile."""
    import torch

    seg_steps = max(args.steps, int(round(0.5 / (ms_region * 1e-3))))
    nseg = max(4, int(np.ceil(args.sustained_seconds / (seg_steps * ms_region * 1e-3))))
    tel = GpuTelemetry(device_index).start()
    idle = None
    pipe.synchronize()
    torch.cuda.synchronize()
    marks = [time.perf_counter()]
    for _ in range(nseg):
        for _ in range(seg_steps):
            step()
        pipe.synchronize()
        marks.append(time.perf_counter())
    tel.stop()
    seg_ms = np.diff(np.asarray(marks)) / seg_steps * 1e3
    total = marks[-1] - marks[0]
    per = int(max(1, round(1.0 / (seg_steps * ms_region * 1e-3))))  # segments per second
    first, last = float(seg_ms[:per].mean()), float(seg_ms[-per:].mean())
    ms = total / (nseg * seg_steps) * 1e3
    out = {"seconds": total, "steps": nseg * seg_steps, "ms_per_step": ms, "value": frames_per_step / (ms * 1e-3), "unit": "frames/s",
           "ms_per_step_first_second": first, "ms_per_step_last_second": last, "ms_per_step_segments": [float(v) for v in seg_ms],
           "segment_steps": seg_steps, "ratio_to_timed_regions": ms / ms_region,
           "telemetry_source": getattr(tel, "source_was", None) or tel.source or f"unavailable ({getattr(tel, 'error', 'no device handle')})",
           "telemetry": {"whole": tel.window(marks[0], marks[-1]), "first_second": tel.window(marks[0], marks[min(per, nseg)]),
                         "last_second": tel.window(marks[max(0, nseg - per)], marks[-1])},
           "note": "one uninterrupted run of the timed loop's steps; a host time stamp (stream synchronisation, no barrier) every segment_steps steps"}
    del idle
    return out


def memory_gb(device):
    """Device memory of this rank at the end of the run (what a rank's share of a sweep needs): torch's peak reserved / allocated bytes
    (workspaces, batches, graph outputs are all torch allocations) and what the driver reports free of the device's total."""
    import torch

    free, total = torch.cuda.mem_get_info(device)
    return {"peak_reserved": torch.cuda.max_memory_reserved(device) / 1e9, "peak_allocated": torch.cuda.max_memory_allocated(device) / 1e9,
            "free_at_end": free / 1e9, "device_total": total / 1e9}


def settle(step, sync, period, seconds):
    """End of the set-up (--settle-seconds): replay the step for about `seconds` of device time before the --warmup steps.  The
    set-up leaves the device mostly idle, and a short timed region right after it runs about 1.5 % slow until clock and power
    management settle (headline, 50-step regions, three runs on one MI355X, not a committed profile: the first region 1.489-1.491 ms,
    the next four 1.465-1.470; `--settle-seconds 0 --repeats 5` shows it).  The count is a multiple of `period` (the streams the
    steps rotate over), so the timed steps read the same batches whatever the count.  Returns the steps replayed (0 if seconds <= 0)."""
    n, chunk = 0, 1
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        t1 = time.perf_counter()
        for _ in range(chunk):
            step()
        sync()
        n += chunk
        chunk = max(1, min(64, int(0.05 / max(1e-6, (time.perf_counter() - t1) / chunk))))  # ~50 ms per synchronisation
    while n % period:
        step()
        n += 1
    sync()
    return n


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: the arrays the timed path returned in its last step, as DIR/<name>.npy in float64 (integer outputs are exact).
    Should they exceed `limit` bytes in all, the arrays whose leading axis is the trial axis (the longest leading axis) keep the same
    fixed, seeded sample of trials, whose numbers go to DIR/sample_rows.npy.  Returns the names written."""
    host = {k: np.ascontiguousarray(np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64))
            for k, v in arrays.items() if v is not None}
    os.makedirs(directory, exist_ok=True)
    if sum(a.nbytes for a in host.values()) > limit:
        n = max(a.shape[0] for a in host.values() if a.ndim)
        per_trial = [k for k, a in host.items() if a.ndim and a.shape[0] == n]
        fixed = sum(a.nbytes for k, a in host.items() if k not in per_trial)
        row_bytes = sum(host[k].nbytes // n for k in per_trial) + 8
        keep = max(1, min(n, (limit - fixed) // row_bytes))
        rows = np.sort(np.random.RandomState(0).choice(n, keep, replace=False))
        for k in per_trial:
            host[k] = np.ascontiguousarray(host[k][rows])
        host["sample_rows"] = rows.astype(np.float64)
    for k, a in host.items():
        np.save(os.path.join(directory, k + ".npy"), a)
    return sorted(host)


def sustained_over_ranks(sustained, grp, device, frames_per_step, ms_region):
    """Like the timed regions: the job's figure is the SLOWEST rank's (every rank ran the same number of steps)."""
    import torch

    if grp.on:
        ts = torch.tensor([sustained["seconds"]], dtype=torch.float64, device=device)
        grp.max_(ts)
        sustained["seconds_this_rank"] = sustained["seconds"]
        sustained["seconds"] = float(ts.item())
        sustained["ms_per_step"] = sustained["seconds"] / sustained["steps"] * 1e3
        sustained["value"] = frames_per_step / (sustained["ms_per_step"] * 1e-3)
        sustained["ratio_to_timed_regions"] = sustained["ms_per_step"] / ms_region
    return sustained


def manifest_entry(relpath):
    """profiles/rNN/MANIFEST.json entry of a committed profile file (tools/make_manifest.py writes them): git SHA, box, command and the
    SHA-256 of the kernel sources the numbers belong to."""
    d = os.path.dirname(os.path.join(ROOT, relpath))
    try:
        man = json.load(open(os.path.join(d, "MANIFEST.json")))
    except (OSError, ValueError):
        return None
    return man.get("files", {}).get(os.path.basename(relpath))


def source_sha256(rel):
    import hashlib

    try:
        return hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest()
    except OSError:
        return None


def run_traffic_child(args):
    """`rocprofv3 --pmc ... -- python3 bench.py --traffic-child`: a few launches of the headline's LIF / beamforming / power stage
    (beamform_ws_kernel at the bench's launch shape) for the counter passes of `live_traffic`.  Random inputs: the stage's HBM traffic
    does not depend on the data (the int8 raster is dense storage), only on the shape."""
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer, neuron_impulse_response

    torch.cuda.set_device(0)
    T, M, fs = TRAFFIC_CHILD_SHAPE  # (live_traffic refuses any other headline shape instead of silently finding no dispatch)
    B, G = args.trials or 1100, args.grid or 360
    tau = 1.0 / (2 * np.pi * 2000.0)
    beamf = SNNBeamformer(geometry=CenterCircularArray(radius=4.5e-2, num_mic=M), kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]),
                          freq_range=[1000.0, 2000.0], fs=fs, bipolar_spikes=True)
    plan = beamf.plan()
    plan.set_neuron_kernel(neuron_impulse_response(np.arange(T) / fs, beamf.tau_vec))
    rng = np.random.RandomState(0)
    W = rng.randn(2 * M, G)
    plan.set_bf_mat(W / np.linalg.norm(W, axis=0, keepdims=True))
    t = np.arange(T) / fs
    x = torch.from_numpy(np.sin(2 * np.pi * 2000 * t)[None, :, None] + rng.randn(B, T, M)).cuda()
    out = plan.snn_pipeline(x, want_power=True)  # fills the workspace's spike raster
    for _ in range(4):
        plan.snn_pipeline(x, stages=4, out=out)
    torch.cuda.synchronize()
    return 0


TRAFFIC_CHILD_SHAPE = (4799, 7, 48_000)  # T, M, fs of `run_traffic_child` (the headline's recording: 0.1 s at 48 kHz, 7 microphones)


def profiler_env_vars(env):
    """Names of the environment variables that say a ROCm profiler's tool library is (pre)loaded into this process tree."""
    out = [k for k in env if k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCP_", "ROCTRACER_", "RPD_"))]
    if any(t in env.get("LD_PRELOAD", "") for t in ("rocprof", "roctracer", "rocprofiler", "librpd")):
        out.append("LD_PRELOAD")
    if "HSA_TOOLS_LIB" in env:
        out.append("HSA_TOOLS_LIB")
    return out


def live_traffic(symbol, B, T, M, G, fs, timeout=240):
    """HBM bytes per launch of the dominant kernel measured IN THIS RUN: two rocprofv3 counter passes (FETCH_SIZE, WRITE_SIZE --
    separate passes, --pmc with the kernel trace only, as MI355X_MICROARCH.md prescribes) over a child that launches the stage at
    the bench's shape; 2 x FETCH_SIZE + WRITE_SIZE (KiB; FETCH_SIZE doubled: the gfx950 correction of the guide).  The child is
    started (never exec'ed) from this process; rocprofv3 is given `python3 bench.py ...` itself.  Returns (bytes or None, detail)."""
    import csv
    import glob
    import shutil
    import tempfile

    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, {"error": "rocprofv3 not found"}
    prof = profiler_env_vars(os.environ)
    if prof:
        # this process already runs under a profiler (its tool library is preloaded): a nested rocprofv3 -- a `#!/usr/bin/env python3`
        # launcher that execs the application -- would be an exec chain from GPU-initialised processes, which this pool forbids
        return None, {"error": "already under a profiler (" + ", ".join(sorted(prof)) + "): live traffic passes skipped"}
    if (T, M, fs) != TRAFFIC_CHILD_SHAPE[:3]:
        return None, {"error": f"live traffic child is built for T, M, fs = {TRAFFIC_CHILD_SHAPE[:3]}, this run has {(T, M, fs)}"}
    tmp = tempfile.mkdtemp(prefix="micloc_pmc_", dir="/tmp")
    vals, detail = {}, {"passes": {}}
    env = dict(os.environ, TMPDIR="/tmp", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    env.pop("MICLOC_FORCE_DIST", None)
    for k in profiler_env_vars(env):  # (none by now; kept so that the child can never inherit a tool library)
        env.pop(k, None)
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, ctr)
            cmd = [exe, "--output-format", "csv", "--kernel-trace", "--pmc", ctr, "-d", d, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--traffic-child", "--trials", str(B), "--grid", str(G)]
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env, cwd="/tmp")
            acc = []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if symbol in r["Kernel_Name"] and r["Counter_Name"] == ctr and int(float(r["Grid_Size"])) == -(-T // 256) * 512 * B:
                        acc.append(float(r["Counter_Value"]))
            detail["passes"][ctr] = {"dispatches": len(acc), "seconds": time.perf_counter() - t0, "rc": p.returncode}
            if not acc:
                detail["error"] = f"no {symbol} dispatch in the {ctr} pass (rc {p.returncode}): " + p.stderr.decode(errors="replace")[-300:]
                return None, detail
            vals[ctr] = float(np.mean(acc))
    except Exception as e:
        detail["error"] = f"{type(e).__name__}: {e}"[:300]
        return None, detail
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    detail.update(fetch_kib=vals["FETCH_SIZE"], write_kib=vals["WRITE_SIZE"],
                  formula="(2 x FETCH_SIZE + WRITE_SIZE) KiB per launch, FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md")
    return (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, detail


class Group:
    """The process group of a run: RCCL (backend "nccl") with one rank per GPU; with --share-device gloo, every collective staged
    through host memory (two ranks cannot share a device under RCCL).  The same calls either way, so the N > 1 code of `run` is one
    code path.  world == 1 without MICLOC_FORCE_DIST: no group, every call is the identity."""

    def __init__(self, rank, world, device, share_device=False, force=False):
        import torch.distributed as dist

        self.dist, self.rank, self.world, self.device = dist, rank, world, device
        self.on = world > 1 or force
        self.staged = bool(share_device)
        self.size = 1
        self.backend = None
        if self.on:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            if self.staged:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
            self.size = dist.get_world_size()
            self.backend = "gloo (host-staged, --share-device rehearsal)" if self.staged else "nccl (RCCL)"

    def barrier(self):
        if self.on:
            self.dist.barrier()

    def gather(self, t):
        """Every rank's `t` (same shape and dtype everywhere), as a list on t's device."""
        if not self.on:
            return [t]
        src = t.cpu() if self.staged else t
        every = [src.new_empty(src.shape) for _ in range(self.world)]
        self.dist.all_gather(every, src.contiguous())
        return [e.to(t.device) for e in every]

    def gather_flat(self, t):
        """ONE collective: the ranks' equal-sized 1-d records concatenated in rank order (all_gather_into_tensor under RCCL)."""
        import torch

        if not self.on:
            return t.clone()
        if self.staged:
            return torch.cat(self.gather(t))
        full = t.new_empty(t.numel() * self.world)
        self.dist.all_gather_into_tensor(full, t)
        return full

    def max_(self, t):
        if self.on:
            if self.staged:
                h = t.cpu()
                self.dist.all_reduce(h, op=self.dist.ReduceOp.MAX)
                t.copy_(h)
            else:
                self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return t

    def gather_object(self, o):
        if not self.on:
            return [o]
        every = [None] * self.world
        self.dist.all_gather_object(every, o)
        return every

    def close(self):
        if self.on:
            self.dist.barrier()
            self.dist.destroy_process_group()


# ----------------------------------------------------------------------------------------------------------------
def run_stub(args, rank, world):
    """Launcher / collective plumbing on CPU (gloo): a few arithmetic 'steps', the same barrier + max-over-ranks timing and
    the same JSON contract.  Not a measurement; used by tests/test_bench_launch_cpu.py only."""
    import torch
    import torch.distributed as dist

    use_dist = world > 1
    if args.steps < 0 and rank == world - 1:
        return 3  # test hook: a rank that dies before the rendezvous
    if use_dist:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    v = torch.arange(1000, dtype=torch.float64)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        v = v * 1.0000001
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    group = 1
    if use_dist:
        dist.barrier()
        dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        group = dist.get_world_size()
    if rank == 0:
        print(json.dumps({"metric": "stub", "value": world * 1000 * args.steps / float(dt.item()), "unit": "elements/s", "n_gpus": group,
                          "rccl_ranks": group, "backend": "gloo (cpu stub)", "steps": args.steps, "warmup": args.warmup, "scaling": "weak"}), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    return 0



# ----------------------------------------------------------------------------------------------------------------
# blocks of the default (noisy, one GPU) line that are not the timed region
# ----------------------------------------------------------------------------------------------------------------
def reference_mae_block(device):
    """'DoA MAE vs ref' of the metric: ONE un-timed pass of the reference's own accuracy sweep
    (paper_plots/target_snn_localization.py:435-467 prints the MAE per SNR at :519-520) in parity mode -- the reference's bf_mat
    (its LAPACK phases, tests/golden/bf_mat_chirp449_bipolar.npz), its global MT19937 stream (np.random.seed(0): rand(1) then
    randn(T, M) per trial), its script-exact grid of 449 DoAs, 11 SNRs x 100 trials -- against the MAE curve the reference
    itself produced on those draws (tests/golden/sweep_full_seed0.npz, generated by tests/golden/make_golden.py)."""
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.sweep import noisy_target_sweep

    gold = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(gold, "sweep_full_seed0.npz"))
    bfz = np.load(os.path.join(gold, "bf_mat_chirp449_bipolar.npz"))
    tau = 1.0 / (2 * np.pi * 2000.0)
    beamf = SNNBeamformer(geometry=CenterCircularArray(radius=4.5e-2, num_mic=7), kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]),
                          freq_range=[1000.0, 2000.0], fs=48_000, bipolar_spikes=True, device=device)
    t0 = time.perf_counter()
    res = noisy_target_sweep(beamf, bfz["bf_mat"], bfz["doa_list"], num_sim=100, seed=int(z["seed"]), mode="parity")
    dt = time.perf_counter() - t0
    return {"mae_ref_deg_per_snr": [float(v) for v in z["mae_deg"]], "mae_deg_per_snr": [float(v) for v in res["mae_deg"]],
            "snr_db": [float(v) for v in z["snr_db_vec"]],
            "max_abs_diff_vs_ref_deg": float(np.max(np.abs(res["mae_deg"] - z["mae_deg"]))),
            "argmax_equal_to_ref": int(np.sum(res["argmax"] == z["argmax"])), "trials": int(z["argmax"].size),
            "max_rel_pmax_diff_vs_ref": float(np.max(np.abs(res["pmax"] / z["pmax"] - 1))),
            "num_doa": int(len(bfz["doa_list"])), "seconds": dt,
            "note": "parity mode, un-timed: the reference's bf_mat fixture, np.random.seed(0) MT19937 stream replayed on the host in the "
                    "reference's draw order, 449-DoA script grid, 11 SNRs x 100 trials; `mae_ref_deg_per_snr` is the reference's own output on "
                    "the same draws (tests/golden/sweep_full_seed0.npz); the timed headline uses Philox noise and a device-designed bf_mat"}


def api_per_call_block(device, calls=40):
    """The unchanged-script path: SNNBeamformer.apply_to_template once per trial, B = 1, the T x G array returned to the
    host (paper_plots/target_snn_localization.py:455; the reference takes 24.7-27.5 ms per trial on 8 vCPUs)."""
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer

    bfz = np.load(os.path.join(ROOT, "tests", "golden", "bf_mat_chirp449_bipolar.npz"))
    tau = 1.0 / (2 * np.pi * 2000.0)
    beamf = SNNBeamformer(geometry=CenterCircularArray(radius=4.5e-2, num_mic=7), kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]),
                          freq_range=[1000.0, 2000.0], fs=48_000, bipolar_spikes=True, device=device)
    time_test = np.arange(0, 100e-3, step=1 / 48_000)
    sig_test = np.sin(2 * np.pi * 2000.0 * time_test)
    np.random.seed(0)
    bf_mat = bfz["bf_mat"]
    snr_db = 5.0 - 10 * np.log10(24.0)

    def one():
        doa = np.random.rand(1)[0] * 2 * np.pi
        t0 = time.perf_counter()
        y = beamf.apply_to_template(bf_mat=bf_mat, template=(time_test, sig_test, doa), snr_db=snr_db)  # the library call
        t1 = time.perf_counter()
        power = np.mean(np.abs(y) ** 2, axis=0)  # the script's own lines :462-464
        am = int(np.argmax(power))
        return y, am, t1 - t0, time.perf_counter() - t1

    for _ in range(3):
        y = one()[0]
    torch.cuda.synchronize()
    ts, tp = [], []
    for _ in range(calls):
        r = one()
        ts.append(r[2])
        tp.append(r[3])
    ts = np.asarray(ts) * 1e3
    tp = np.asarray(tp) * 1e3
    return {"apply_to_template_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "calls": calls,
            "script_power_argmax_ms": float(np.median(tp)), "trial_ms": float(np.median(ts + tp)),
            "returns": f"numpy float64 [{y.shape[0]} x {y.shape[1]}] on the host ({y.nbytes / 1e6:.1f} MB D2H per call into a page-locked block)",
            "frames_per_s": float(y.shape[0] / (np.median(ts + tp) * 1e-3)),
            "reference_ms_per_trial": "24.7-27.5 (8 vCPU Xeon 2.1 GHz, SURVEY 6)",
            "note": "one trial per call exactly as the script's loop does it.  apply_to_template_ms = the library call: host synthesis + host MT19937 noise "
                    "(reference draw order), H2D, STHT -> RZCC -> LIF -> beamforming with y stored, D2H of T x G; script_power_argmax_ms = the caller's "
                    "own np.mean(np.abs(y)**2) / np.argmax on the returned array; trial_ms = both.  PCIe- and host-bound, never `value`"}


def beamformer_c128_block(wl, args):
    """SURVEY 8a row a11 -- the NON-spiking Beamformer (micloc/beamformer.py:260-292: STHT, band-pass, sig @ conj(bf_mat), the dense
    steering-matrix x analytic-signal contraction) on the headline's batch and grid: `Beamformer.localize_batch`'s pipeline
    (power / arg-max, no T x G temporary) captured per stream like the headline, the contraction kernel alone (HIP events), and the
    API-faithful form that stores apply_to_signal's T x G complex128 array (16 G bytes per frame: HBM-write bound)."""
    import torch

    from haghighatshoarmuir2024_amd import runtime
    from haghighatshoarmuir2024_amd.beamformer import Beamformer

    x = wl["x"]
    B, T, M = x.shape
    G = wl["bf_mat"].shape[1]
    dev = x.device
    sb = wl["beamf"]
    bm = Beamformer(geometry=sb.geometry, kernel_duration=sb.kernel_duration, freq_range=wl["freq_range"], fs=sb.fs, device=dev)
    doa_list = np.linspace(-np.pi, np.pi, G)
    t0 = time.perf_counter()
    bf_mat, _ = bm.design_from_template(chirp_template(sb.fs, wl["freq_range"]), doa_list, svd="device")
    torch.cuda.synchronize()
    t_design = time.perf_counter() - t0
    b, a = bm.bandpass_filter
    plans = [runtime.Plan(M, bm.kernel, b, a, 1, False, device=dev) for _ in range(max(1, args.streams))]
    for p in plans:
        p.set_bf_mat(bf_mat)
    pipe = runtime.StreamPipeline(plans)
    replay = pipe.capture(lambda plan: plan.beamformer_pipeline(x, want_y=False, want_power=True))

    fn = replay  # (timed below with THIS pipeline's streams in the bracket, single rank: the variant is reported at N = 1 only)

    pipe.synchronize()
    for _ in range(args.warmup):
        fn()
    times = []
    for _ in range(3):
        pipe.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        pipe.synchronize()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))

    def ev(fn_, iters=10, inner=2):
        fn_()
        torch.cuda.synchronize()
        e0 = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        e1 = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
        for i in range(iters):
            e0[i].record()
            for _ in range(inner):
                fn_()
            e1[i].record()
        torch.cuda.synchronize()
        return float(np.mean([a_.elapsed_time(b_) for a_, b_ in zip(e0, e1)])) / inner

    plan = plans[0]
    h = plan.stht(x)
    pre, _ = plan.bandpass_rzcc(h, T, want_pre=True, want_spikes=False)
    del h
    o = plan.beamform_c128(pre, T, want_y=False, want_power=True)
    ms_k = ev(lambda: plan.beamform_c128(pre, T, out=o))
    same = bool(torch.equal(o["argmax"], out["argmax"]))
    flop = 8 * M * G + 4 * G
    ach = B * T * flop / (ms_k * 1e-3) / 1e12
    res = {"ms_per_step": dt / args.steps * 1e3, "value": B * T * args.steps / dt, "unit": "frames/s",
           "workload": f"Beamformer.localize_batch: {B} trials x {T} frames x {M} mics, {G}-DoA complex bf_mat (designed on the device, {t_design:.2f} s), "
                       f"STHT -> band-pass -> sig @ conj(bf_mat) -> mean|y|^2 -> arg-max; {len(plans)} HIP streams, graphs",
           "roofline": {"kernel": "beamform_wsc_kernel", "bound": "mfma", "achieved": ach, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": ach / FP64_MFMA_PEAK_TFLOPS, "avg_launch_ms": ms_k, "flop_per_frame": flop,
                        "note": "8 M G (complex multiply-adds of sig @ conj(bf_mat)) + 4 G (|y|^2) flop per frame; HIP events around the launch + power_argmax_kernel"},
           "argmax_stage_equal_to_pipeline": same}
    # API-faithful: y [B, T, G] complex128 stored (apply_to_signal's return value), in batches that fit 24 GB
    By = max(1, min(B, int(24e9 // (T * G * 16))))
    oy = plan.beamform_c128(pre[:By], T, want_y=True, want_power=False)
    ms_y = ev(lambda: plan.beamform_c128(pre[:By], T, out=oy), iters=5, inner=1)
    gbs = By * T * (16 * G + 8 * 2 * M) / (ms_y * 1e-3) / 1e9
    res["y_stored"] = {"ms_per_launch": ms_y, "trials": By, "frames_per_s": By * T / (ms_y * 1e-3), "bytes_per_frame": 16 * G + 16 * M,
                       "roofline": {"kernel": "beamform_wsc_kernel<.., WANT_Y>", "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": gbs / HBM_PEAK_GBS},
                       "note": "apply_to_signal's T x G complex128 result written to HBM (16 G bytes per frame) + the planar input read (16 M)"}
    del oy, pre
    return res


def streaming_live_block(wl):
    """The reference's live loop (micloc/localization_demo_snn.py:125-193: a 0.25 s frame of 12 000 samples, the chain, a DoA) as a
    stream: StreamingLocalizer on one recording, tiles of 12 000 frames, eager push() against push_replay() (ONE hipGraph launch per
    tile: the stream's clock lives on the device).  Reports the wall time per tile with the device drained after every tile (what a
    live consumer sees), and that both give the same running estimate."""
    import torch

    from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

    beamf, bf_mat = wl["beamf"], wl["bf_mat"]
    n, tiles = 12_000, 24
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.randn(1, n * tiles, len(beamf.geometry))).to(wl["x"].device)
    out = {}
    ref = None
    for mode in ("push", "push_replay"):
        s = StreamingLocalizer(beamf, bf_mat, 1, max_tile=n, lag_frames=4096)
        fn = getattr(s, mode)
        ts = []
        for k in range(tiles):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p, a = fn(x[:, k * n : (k + 1) * n, :])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[mode + "_ms_per_tile"] = float(np.median(ts[4:]) * 1e3)  # (the first tiles include the capture)
        st = s.status()
        if ref is None:
            ref = (p.clone(), a.clone(), st)
        else:
            out["same_estimate"] = bool(torch.equal(ref[0], p) and torch.equal(ref[1], a) and ref[2] == st)
    out["tile_frames"] = n
    out["realtime_factor"] = 0.25 / (out["push_replay_ms_per_tile"] * 1e-3)
    out["note"] = ("one recording, 0.25 s tiles (12 000 frames x 7 mics), wall time per tile incl. the H2D-free hand-over and a device "
                   "synchronisation; push_replay = one captured hipGraph per tile (DESIGN.md 4.2)")
    return out


def other_configs_block(args):
    """The other BASELINE configs on the same box, a few steps each, as CHILD processes of this (GPU-initialised) process --
    started, never exec'ed; one at a time."""
    out = {}
    # the headline once more with this process's children pinned to TWO host cores: at 8 ranks a 16-core cgroup leaves each rank two,
    # and 3 streams of graph replays per rank must not become host bound there
    try:
        cmd = [sys.executable, os.path.abspath(__file__), "--cpu-cores", "2", "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", "3",
               "--no-cpu-baseline", "--no-other-configs", "--streams", str(args.streams), "--sustained-seconds", "0"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
        d = json.loads([ln for ln in p.stdout.decode(errors="replace").splitlines() if ln.startswith("{")][-1])
        out["noisy_on_2_host_cores"] = {"ms_per_step": d["ms_per_step"], "value": d["value"], "cpu_cores": d["cpu_cores_per_rank"],
                                        "note": "the default workload with the process pinned to 2 host cores (--cpu-cores 2): a rank's share at 8 ranks per 16-core cgroup"}
    except Exception as e:
        out["noisy_on_2_host_cores"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    # (enough steps per timed region for the three streams to drift out of step: with one step per stream they start together and
    #  finish together, which is not the steady state -- xylo 18.0 ms/step at 3 steps, 17.0 at 12)
    for cfg, steps in (("speech", 16), ("xylo", 12), ("stress", 9)):
        cmd = [sys.executable, os.path.abspath(__file__), "--config", cfg, "--steps", str(steps), "--warmup", "4" if cfg == "speech" else "3", "--repeats", "3",
               "--full", "--no-cpu-baseline", "--no-other-configs", "--sustained-seconds", str(args.other_sustained_seconds)] + \
              (["--streams", str(args.streams)] if args.streams_given else [])
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
            lines = [ln for ln in p.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
            d = json.loads(lines[-1])
            r = d["roofline"]
            out[cfg] = {"ms_per_step": d["ms_per_step"], "value": d["value"], "unit": "frames/s", "workload": d["config"]["workload"],
                        "schedule": d["config"].get("schedule"),
                        "roofline": {k: r.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms")},
                        "stages_ms": r.get("stages_ms"), "steps": d["steps"], "wall_s": time.perf_counter() - t0}
            sus = d.get("sustained")
            if sus:
                # the steady state of the workload: ONE uninterrupted region (no fill / drain per K steps) with the chip's own telemetry
                out[cfg]["sustained"] = {k: sus.get(k) for k in ("seconds", "steps", "ms_per_step", "value", "unit", "ms_per_step_first_second",
                                                                 "ms_per_step_last_second", "ratio_to_timed_regions", "telemetry_source")}
                out[cfg]["sustained"]["telemetry"] = (sus.get("telemetry") or {}).get("whole")
                out[cfg]["sustained"]["ms_per_step_segments_min_max"] = [min(sus["ms_per_step_segments"]), max(sus["ms_per_step_segments"])]
            if "parity" in d:
                out[cfg]["parity"] = "unpinned"
                out[cfg]["parity_note"] = d["parity"]
        except Exception as e:  # a failed child run is reported, it does not take the headline line down
            out[cfg] = {"error": f"{type(e).__name__}: {e}"[:300]}
    return out


XYLO_VALU_PER_WAVE_STEP = 20  # vector instructions per wave (128 neurons, two per lane) and time step: 18 of the packed update +
#                               2 v_perm that pair the matrix-core currents (ISA of xylo_lif_pk_kernel<1, false>)


def run_xylo(args, rank, local_rank, world):
    """BASELINE configs[3]: the Xylo sweep of paper_plots/target_xylo_localization.py:540-608 as a throughput run.
    One step = STHT -> order-1 band-pass -> RZCC -> integer LIF hidden layer (spike counts only) -> find_peak_location ->
    DoA error for a batch of trials resident in HBM.  PARITY UNPINNED for the LIF stage (rockpool / XyloSim absent)."""
    import torch
    import torch.distributed as dist

    from haghighatshoarmuir2024_amd import runtime, synthesis
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo

    dev_index = 0 if args.share_device else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    grp = Group(rank, world, device, share_device=args.share_device)
    use_dist = grp.on
    group_size = grp.size
    fs, M = 48_000, 7
    G = args.grid or 360
    B = args.trials or 1100
    geometry = CenterCircularArray(radius=4.5e-2, num_mic=M)
    doa_list = np.linspace(-np.pi, np.pi, G)
    f_min, f_max = 1000.0, 2000.0
    demo = Demo(geometry=geometry, freq_bands=[[f_min, f_max]], doa_list=doa_list, recording_duration=0.25, bipolar_spikes=True, fs=fs, device=device)
    time_test = np.arange(0, 1000e-3, step=1 / fs)  # target_xylo_localization.py:549-560
    period = time_test[-1]
    sig_test = np.sin(2 * np.pi * np.cumsum(f_min + (f_max - f_min) * (time_test % period) / period) / fs)
    rng = np.random.RandomState(2000 + rank)
    doa = rng.rand(B) * 2 * np.pi
    snr_db_vec = np.linspace(-10, 20, 11)
    groups = len(snr_db_vec) if B % len(snr_db_vec) == 0 else 1
    snr_db = snr_db_vec[(np.arange(B) * len(snr_db_vec)) // B] - 10 * np.log10((fs / 2) / (f_max - f_min))
    x = synthesis.signal_from_template_batch(geometry, (time_test, sig_test), doa, device=device, device_delays=True)
    synthesis.add_noise_(x, snr_db, seed=4321, first_trial=rank * B)
    T = x.shape[1]
    win = 2 * ((G // 32) // 2) + 1
    d_doa = torch.from_numpy(doa).to(device)
    d_list = torch.from_numpy(doa_list).to(device)
    net = demo.network()  # quantised weights resident on the device, shared (read-only) by all streams
    plan = demo._plans()[0]
    enc = demo.beamfs[0].spk_encoder
    bb, aa = demo.filterbank.ba_list[0]
    nstreams = max(1, args.streams)
    # consecutive steps are independent batches: the latency-bound encoder of one overlaps the issue-bound LIF of another
    plans = [plan] + [runtime.Plan(M, demo.beamfs[0].kernel, bb, aa, enc.robust_width, enc.bipolar, device=device) for _ in range(nstreams - 1)]
    if args.encoder_chunk is not None:
        for pl in plans:
            pl.set_encoder_chunk(args.encoder_chunk)
    pipe = runtime.StreamPipeline(plans)

    lif_kw = dict(queued=False) if args.xylo_lif == "static" else dict(queued=True, workers_per_cu=int((args.xylo_lif.split(":") + ["0"])[1]))

    def body(pl):
        # STHT + band-pass + RZCC of the fused pipeline (Demo.raster_device): only the quadrature rows go through HBM, the encoder reads
        # the in-phase ones -- the rolled input frames -- from x itself
        raster = pl.snn_pipeline(x, want_spikes=True, want_power=False, stages=3)["spikes"]
        counts = net.run(raster, ternary=True, **lif_kw)[1]  # the +/- split of spike_encoding happens in the kernel's staging loop
        idx = runtime.peak_location(counts, G, win)
        _, mae = runtime.doa_error(idx, d_list, d_doa, groups=groups, want_err=False)
        return counts, idx, mae

    replay = pipe.capture(body)
    keepalive = (x, d_doa, d_list, plans, net)  # noqa: F841  (everything the captured graphs read)

    def barrier():
        pipe.synchronize()
        grp.barrier()
        torch.cuda.synchronize()

    settle_steps = settle(replay, pipe.synchronize, nstreams, args.settle_seconds)
    for _ in range(args.warmup):
        replay()
    dt_all = []
    per_rank = []
    for _ in range(max(1, args.repeats)):
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            counts, idx, mae = replay()
        barrier()
        dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
        per_rank.append([float(v.item()) for v in grp.gather(dt)])
        grp.max_(dt)
        dt_all.append(float(dt.item()))
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"counts": counts, "peak_index": idx, "mae": mae})  # the last step's outputs (this rank's MAE)
    mae = torch.stack(grp.gather(mae)).mean(dim=0)
    dt = float(np.median(dt_all))
    frames = group_size * B * T * args.steps
    sustained = None
    if args.sustained_seconds > 0:
        barrier()
        sustained = sustained_block(lambda: replay(), pipe, args, dt / args.steps * 1e3, group_size * B * T, dev_index)
        sustained = sustained_over_ranks(sustained, grp, device, group_size * B * T, dt / args.steps * 1e3)
        barrier()
    result = None
    roof = queue_gave_up = None
    if rank == 0 and args.full:
        def timed(fn, iters=5):
            fn()
            torch.cuda.synchronize()
            e0 = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
            e1 = [torch.cuda.Event(enable_timing=True) for _ in range(iters)]
            for i in range(iters):
                e0[i].record()
                fn()
                e1[i].record()
            torch.cuda.synchronize()
            return float(np.mean([a.elapsed_time(b) for a, b in zip(e0, e1)]))

        stage_out = plan.snn_pipeline(x, want_spikes=True, want_power=False, stages=3)
        raster = stage_out["spikes"]
        st = {"stht_kernel": timed(lambda: plan.snn_pipeline(x, want_spikes=True, want_power=False, stages=1, out=stage_out)),
              "bandpass_rzcc_kernel": timed(lambda: plan.snn_pipeline(x, want_spikes=True, want_power=False, stages=2, out=stage_out)),
              "xylo_lif_kernel": timed(lambda: net.run(raster, ternary=True, **lif_kw)),
              "xylo_lif_queue_alone": timed(lambda: net.run(raster, ternary=True, queued=True)),
              "peak_location_kernel": timed(lambda: runtime.peak_location(counts, G, win))}
        queue_gave_up = net.queue_status()["gave_up"]  # (of the stand-alone queue launch just timed: must be 0)
        dom = max((k for k in st if k != "xylo_lif_queue_alone"), key=st.get)
        N = net.N
        nblocks = -(-N // 512)
        waves_per_trial = 4 * nblocks if nblocks > 1 else -(-N // 128)
        waves = waves_per_trial * B
        lif_ginstr = waves * T * XYLO_VALU_PER_WAVE_STEP / (st["xylo_lif_kernel"] * 1e-3) / 1e9
        valu_peak = 1024 * 2.4 / 4  # SIMDs x GHz / cycles per wave instruction
        lif_note = (f"{XYLO_VALU_PER_WAVE_STEP} vector instructions per wave and time step, {waves} waves x {T} steps over 1024 SIMDs "
                    f"({waves / 1024:.2f} per SIMD: the busiest holds {-(-waves // 1024)}); lanes used {N}/{waves_per_trial * 128} x 2 neurons")
        if dom == "xylo_lif_kernel":
            # integer recurrences, two neurons per lane, sequential in time: bound by vector-instruction issue (4 cycles per wave
            # instruction per SIMD), neither HBM (14 B of input per frame) nor MFMA (8 int8 MFMAs per 16 steps and wave)
            roof = dict(kernel="xylo_lif_pk_kernel", bound="valu-issue (integer recurrences; neither HBM nor MFMA binds)", achieved=lif_ginstr,
                        peak=valu_peak, unit="G wave-instructions/s", frac=lif_ginstr / valu_peak, traffic=None, note=lif_note)
        else:
            achieved = B * T * (8 * 2 * M + 2 * M) / (st[dom] * 1e-3) / 1e9
            roof = dict(kernel=dom, bound="hbm", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s", frac=achieved / HBM_PEAK_GBS, traffic=None,
                        note="the band-pass / RZCC stage is a serial chain per (trial, channel) stream -- latency bound on one wave per 64 streams, "
                             "data dependent (the order-1 band-pass of this configuration passes ~3x the peak candidates of the order-2 one: 1.0 "
                             "instead of 0.34 ms per 4800 frames) -- and occupies few SIMD cycles; in the pipelined step it runs beside the "
                             "other stages.  The stage that fills the SIMDs is the integer LIF: "
                             f"{lif_ginstr:.0f} of {valu_peak:.0f} G wave-instructions/s = {lif_ginstr / valu_peak:.2f} of the issue bound; " + lif_note)
        roof["avg_launch_ms"] = st[dom]
        roof["stages_ms"] = st
    if rank == 0:
        value = frames / dt
        result = {
            "metric": "audio samples/sec through STHT+RZCC+SNN beamform, 7-mic 48kHz 360-DoA; DoA MAE vs ref",
            "value": value, "unit": "frames/s (one frame = one audio sample instant across all mics)",
            "n_gpus": group_size, "rccl_ranks": group_size if (use_dist and not grp.staged) else 0, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "ms_per_step_repeats": [t / args.steps * 1e3 for t in dt_all],
            "ms_per_step_per_rank": (np.median(np.asarray(per_rank), axis=0) / args.steps * 1e3).tolist(),
            "timing_note": f"median of {len(dt_all)} timed regions of exactly {args.steps} steps each (barrier + synchronize on both sides, max over "
                           f"ranks), after {settle_steps} settle steps (--settle-seconds {args.settle_seconds:g}) and {args.warmup} warm-up steps",
            "cpu_cores_per_rank": args.cpu_cores or usable_cores(),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64 encoder + int16 LIF state / int8 weights", "data": "synthetic",
            "parity": "UNPINNED for the integer-LIF stage (rockpool / XyloSim absent); spike encoding and peak finding pinned",
            "config": {"workload": f"target_xylo_localization sweep (Xylo-A2 integer LIF, bipolar RZCC): {M}-mic, {fs // 1000} kHz, T={T} (1 s chirp), "
                                   f"{B} trials/GPU/step, {G} hidden neurons = DoA grid, {4 * M} input channels, find_peak_location(win={win})",
                       "trials_per_gpu": B, "frames_per_trial": T, "num_mic": M, "num_doa": G, "mic_samples_per_s": value * M,
                       "parallelism": f"trial-sharded x{group_size}", "hip_streams": nstreams, "hip_graphs": True,
                       "w_rec_quantised": int(net.w_rec), "lif_launch": args.xylo_lif, "settle_steps": settle_steps},
            "mae_deg_per_snr": [float(v) for v in (mae * 180 / np.pi).cpu().numpy()],
        }
        if roof is not None:
            result["roofline"] = roof
            result["config"]["lif_queue_workers_gave_up"] = int(queue_gave_up)
        if sustained is not None:
            result["sustained"] = sustained
            result["config"]["sustained_ms_per_step"] = sustained["ms_per_step"]
        if grp.backend:
            result["backend"] = grp.backend
    grp.close()
    if rank == 0:
        sys.stdout.flush()
        print(json.dumps(result), flush=True)
    return 0


def run(args):
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if args.cpu_stub:
        return run_stub(args, rank, world)
    if args.traffic_child:
        return run_traffic_child(args)
    np_pool, np_workers = None, 0
    if args.full and args.config == "noisy" and world == 1 and rank == 0 and not args.no_cpu_baseline and os.environ.get("MICLOC_FORCE_DIST") != "1":
        # the NumPy leg's worker processes: started while this process is still GPU-free (nothing above touched HIP)
        try:
            np_workers = usable_cores()
            np_pool = numpy_pool(np_workers)
        except Exception as e:
            print(f"bench.py: numpy_ops_all_cores leg unavailable ({type(e).__name__}: {e})", file=sys.stderr)
            np_pool, np_workers = None, 0
    import torch
    import torch.distributed as dist

    if world != args.gpus and world > 1:
        args.gpus = world
    args.world = world
    dev_index = 0 if args.share_device else local_rank
    if dev_index >= torch.cuda.device_count():
        print(f"bench.py: rank {rank} has no device (LOCAL_RANK {local_rank}, {torch.cuda.device_count()} visible)", file=sys.stderr)
        return 2
    if args.config == "xylo":
        return run_xylo(args, rank, local_rank, world)
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    # MICLOC_FORCE_DIST=1 runs the collective code path with a 1-rank RCCL group (to exercise it on a 1-GPU box)
    grp = Group(rank, world, device, share_device=args.share_device, force=os.environ.get("MICLOC_FORCE_DIST") == "1")
    use_dist = grp.on
    group_size = grp.size

    wl = build_workload(args, rank if args.as_rank is None else args.as_rank, device)
    noisy = args.config == "noisy"
    # consecutive steps are independent batches: on every workload the serial scan / encoder of one step (few, long
    # latency-bound workgroups) overlaps the throughput-bound STHT and beamforming kernels of its neighbours
    nstreams = max(1, args.streams)
    # every stream holds its own batch, end-to-end copy and workspace: fewer streams rather than an out-of-memory kill when a
    # rank's share is large (--baseline-total on few GPUs)
    per_stream = 2 * wl["x"].numel() * 8 + wl["plan"].lib.micloc_workspace_bytes(wl["plan"].handle, wl["x"].shape[0], wl["x"].shape[1])
    free_bytes = torch.cuda.mem_get_info(device)[0]
    while nstreams > 1 and (nstreams - 1) * per_stream > 0.6 * free_bytes:
        nstreams -= 1
    if nstreams == 1 and 1.2 * wl["x"].numel() * 8 > free_bytes:  # (the end-to-end variant keeps a second copy of the batch)
        print(f"bench.py: {wl['x'].shape[0]} trials per rank need about {per_stream / 1e9:.0f} GB per stream, {free_bytes / 1e9:.0f} GB are free: "
              "use --trials or more GPUs", file=sys.stderr)
        return 2
    # long recordings: the encoder's serial scan on a stream with compute units of its own (when the encoder is time-chunked at all)
    scan_lane = args.scan_lane_cus if (args.schedule == "scan-lane" and nstreams > 1 and
                                       wl["plan"].encoder_chunks(wl["x"].shape[0], wl["x"].shape[1]) > 1) else 0
    # a plain run captures the headline step only; --full adds the covariance / fp32 variants and the end-to-end step
    variants = (True if noisy else None) if args.full else False
    try:
        step, pipe = make_step(wl, nstreams, variants=variants, scan_lane=scan_lane, e2e=args.full)
    except Exception as e:  # (a box that refuses compute-unit masks: the schedule is an optimisation, not a requirement)
        if not scan_lane:
            raise
        print(f"bench.py: scan-lane schedule unavailable ({type(e).__name__}: {e}); falling back to graphs", file=sys.stderr)
        scan_lane = 0
        step, pipe = make_step(wl, nstreams, variants=variants, scan_lane=0, e2e=args.full)
    B, T, M = wl["x"].shape
    G = wl["bf_mat"].shape[1]

    def barrier():
        pipe.synchronize()
        grp.barrier()
        torch.cuda.synchronize()

    per_rank = []  # one list per timed region (headline regions first)

    def timed_steps(fn, repeats=1):
        """W warm-up steps, then `repeats` timed regions of EXACTLY K steps, each bracketed by barrier + synchronize on both
        sides and reduced with MAX over ranks.  Returns (median seconds per region, all regions, last result)."""
        for _ in range(args.warmup):
            fn()
        times = []
        res = None
        for _ in range(max(1, repeats)):
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                res = fn()
            barrier()
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device)
            per_rank.append([float(v.item()) for v in grp.gather(t)])  # every rank's own clock: a straggler shows up by name, not only in the MAX
            grp.max_(t)
            times.append(float(t.item()))
        return float(np.median(times)), times, res

    settle_steps = settle(step, pipe.synchronize, nstreams, args.settle_seconds)
    dt, dt_all, (out, mae) = timed_steps(step, args.repeats)
    if rank == 0 and args.dump_outputs:
        # what the timed path returned in its last step (graph outputs are static buffers: before anything else replays them)
        dump_outputs(args.dump_outputs, {"power": out["power"], "argmax": out["argmax"], "mae": mae})
    ms_per_rank = (np.median(np.asarray(per_rank[: len(dt_all)]), axis=0) / args.steps * 1e3).tolist()
    exchange = None
    uuids = [str(getattr(torch.cuda.get_device_properties(device), "uuid", "n/a"))]
    if use_dist and args.full:
        # the sweep's one exchange step (ref:paper_plots/target_snn_localization.py:447-467 keeps doa / arg-max per trial): every
        # rank's per-trial {doa f64, p_max f64, argmax i32} of its last step as ONE struct-of-arrays record, one all_gather_into_tensor
        # (RCCL over xGMI), timed between two barriers; rank 0 recomputes the MAE per SNR from the gathered trials
        out0, mae0 = step(index=0)  # (stream 0's batch: wl["x"] with the DoAs wl["doa"])
        pipe.synchronize()
        mae0 = (mae0 * 180 / np.pi).cpu().numpy()
        doa0 = wl["doa"]
        rec = torch.empty(3 * B, dtype=torch.float64, device=device)
        ex_ms = []
        for _ in range(5):
            barrier()
            t0 = time.perf_counter()
            rec[:B] = doa0
            rec[B : 2 * B] = out0["power"].gather(1, out0["argmax"].long().view(-1, 1)).view(-1)
            rec[2 * B :].view(torch.int32)[:B] = out0["argmax"]
            host = grp.gather_flat(rec).cpu()  # RCCL: one all_gather_into_tensor + one D2H; rehearsal: D2H, gloo all_gather, concatenate
            ex_ms.append((time.perf_counter() - t0) * 1e3)
        host = host.view(world, 3, B)
        g_doa = host[:, 0, :].numpy()
        g_am = host[:, 2, :].contiguous().view(torch.int32)[:, :B].numpy()
        g_err = np.arcsin(np.abs(np.sin(wl["doa_list"].cpu().numpy()[g_am] - g_doa)))  # :466
        S_ = wl["snr_groups"]
        mae_gathered = g_err.reshape(world, S_, B // S_).mean(axis=(0, 2)) * 180 / np.pi
        exchange = {"exchange_ms": float(np.median(ex_ms)), "exchange_ms_all": [float(v) for v in ex_ms], "collectives": 1,
                    "bytes_per_rank": int(rec.numel() * 8), "record": "{doa f64, p_max f64, argmax i32} x trials, struct of arrays",
                    "mae_deg_per_snr_from_gathered_trials": [float(v) for v in mae_gathered],
                    "mae_deg_per_snr_device_same_batch": [float(v) for v in mae0],  # rank 0's own batch by micloc_doa_error_f64
                    "transport": grp.backend,
                    "note": "pack on the device + one all_gather_into_tensor + one D2H, between two barriers; not inside the timed steps "
                            "(a sweep exchanges once, at its end)"}
    if use_dist:
        uuids = [str(u) for u in grp.gather_object(uuids[0])]
        mae = torch.stack(grp.gather(mae)).mean(dim=0)
    frames = group_size * B * T * args.steps
    value = frames / dt
    sustained = None
    if args.sustained_seconds > 0:
        # every rank runs it (the same load on every GPU of the node); rank 0 reports its own.  Under the scan-lane schedule (long
        # recordings) the region is the same eager launches the timed regions make: what it adds is the steady state -- a K-step
        # region of a four-deep pipeline with an 8 ms serial scan in front is mostly fill and drain
        barrier()
        sustained = sustained_block(step, pipe, args, dt / args.steps * 1e3, group_size * B * T, dev_index)
        sustained = sustained_over_ranks(sustained, grp, device, group_size * B * T, dt / args.steps * 1e3)
        barrier()
    e2e = cov_variant = f32_variant = argmax_direct = None
    if args.full:
        # comparisons between the variants and with the CPU baseline use stream 0's batch (wl["x"]): every stream has its own trials
        out, _ = step(index=0)
        pipe.synchronize()
        argmax_direct = out["argmax"].clone()  # graph outputs are static buffers: keep a copy for the comparisons below
        power_direct = out["power"].clone()

        # the same K steps with the input side inside the graph (synthesis + noise regenerated every step)
        dte, _, (out_e, mae_e) = timed_steps(lambda: step(cov="e2e"), min(args.repeats, 3))
        mae_e = torch.stack(grp.gather(mae_e)).mean(dim=0)
        e2e = {"value": frames / dte, "unit": "frames/s", "ms_per_step": dte / args.steps * 1e3,
               "mae_deg_per_snr": [float(v) for v in (mae_e * 180 / np.pi).cpu().numpy()],
               "note": "per step, inside the same HIP graph: DoA draw (Philox), delayed-template synthesis with in-kernel delays fused with the AWGN "
                       "(Philox + Box-Muller at the trial's SNR; the noise-free signal is never stored), then the hot path and the DoA error; "
                       "fresh trials every step"}

        if M * 2 <= 128:
            # separately reported algorithmic variant: covariance-form power, same K steps, same inputs
            dtc, _, _ = timed_steps(lambda: step(cov=True))
            out_c, _ = step(cov=True, index=0)
            pipe.synchronize()
            cov_variant = {"value": frames / dtc, "unit": "frames/s", "ms_per_step": dtc / args.steps * 1e3,
                           "argmax_equal_to_direct": bool(torch.equal(out_c["argmax"], argmax_direct)),
                           "max_rel_power_diff_vs_direct": float((out_c["power"] / power_direct - 1).abs().max().item()),
                           "note": "power = w^T (V^T V / T) w instead of mean_t (V w)^2: algebraically identical, 2C^2 instead of 2CG flops per frame; not the headline"}
        if noisy and M * 2 <= 64:
            # second separately reported variant: fp32-MFMA beamforming tail (fp64 up to the spikes)
            dtf, _, _ = timed_steps(lambda: step(cov="f32"))
            out_f, _ = step(cov="f32", index=0)
            pipe.synchronize()
            relerr = float((out_f["power"] / power_direct - 1).abs().max().item())
            f32_variant = {"value": frames / dtf, "unit": "frames/s", "ms_per_step": dtf / args.steps * 1e3,
                           "argmax_equal_to_f64": int((out_f["argmax"] == argmax_direct).sum().item()), "trials": int(B),
                           "max_rel_power_err_vs_f64": relerr,
                           "note": "LIF + beamforming + power on v_mfma_f32_16x16x4_f32 (157 TF peak); STHT / band-pass / RZCC stay fp64; not the headline"}

    result = None
    if rank == 0:
        roof = None
        if args.full:
            # the per-kernel stage times (runs of their own) and the roofline of the dominant kernel
            st = stage_times(wl, max(5, min(args.steps, 20)))
            n_nir = len(wl["nir"])
            C = 2 * M
            # algorithmic work per frame (SURVEY 8d / DESIGN.md): dense-tap STHT as the reference computes it
            flops = {
                "stht_kernel": 2 * len(wl["beamf"].kernel) * M,
                "bandpass_rzcc_kernel": 17 * C,
                "beamform_kernel": 2 * n_nir * C + 2 * C * G + 2 * G,
            }
            dom = max(st, key=st.get)
            frames_launch = B * T
            traffic_src = None
            serial_stage = None
            if dom == "bandpass_rzcc_kernel":
                # The longest BRACKET is the band-pass / RZCC stage: a serial dependency chain per (trial, channel) stream (DF2T +
                # running sum; long streams are cut into chunks behind a serial scan, rzcc_scan_kernel, on a handful of CUs).  It is
                # latency, not throughput, and in the pipelined step it runs beside the neighbouring steps' kernels -- it sits on no
                # roof.  The roofline object therefore prices the dominant THROUGHPUT kernel; the stage is reported beside it.
                serial_stage = {"stage": "bandpass_rzcc", "ms": st[dom], "algorithmic_GBs": frames_launch * (8 * C + C) / (st[dom] * 1e-3) / 1e9,
                                "encoder_chunks": int(wl["plan"].encoder_chunks(B, T)),
                                "note": "serial-latency stage (scan + chunked encoder), overlapped with the other kernels of neighbouring steps; see DESIGN.md 4.2"}
                dom = max((k for k in st if k != "bandpass_rzcc_kernel"), key=st.get)
            achieved = frames_launch * flops[dom] / (st[dom] * 1e-3) / 1e12
            traffic = args.traffic_bytes
            traffic_detail = None
            if traffic is None and dom == "beamform_kernel" and C <= 16:
                # launch size of beamform_ws_kernel: 256-frame chunks x 512 work-items per trial
                if noisy and group_size == 1 and not args.no_live_traffic and not args.no_other_configs:
                    torch.cuda.synchronize()
                    traffic, traffic_detail = live_traffic(KERNEL_SYMBOL[dom], B, T, M, G, wl["fs"])
                    traffic_src = "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over a child of this run (bench.py --traffic-child)"
                if traffic is None:
                    # a COMMITTED profile -- only if its MANIFEST says it was taken on the kernel source this run executes
                    t2, src = traffic_from_profiles(KERNEL_SYMBOL[dom], -(-T // 256) * 512 * B, args.pmc_summary)
                    ent = manifest_entry(src) if src else None
                    cur = source_sha256("haghighatshoarmuir2024_amd/csrc/beamform.hip")
                    if t2 is not None and ent and ent.get("sources_sha256", {}).get("haghighatshoarmuir2024_amd/csrc/beamform.hip") == cur:
                        traffic, traffic_src = t2, f"{src} (MANIFEST: git {ent.get('git_sha', '?')[:10]}, csrc/beamform.hip unchanged since)"
                    else:
                        traffic_src = (f"none: {src} has no MANIFEST entry for the current csrc/beamform.hip (stale or unlisted profile refused)"
                                       if src else "none: no committed PMC summary")
            sym = KERNEL_SYMBOL.get(dom, dom)
            if dom == "beamform_kernel" and C > 16:
                sym = "beamform_gen_kernel"
            roof = dict(kernel=sym, bound="mfma", achieved=achieved, peak=FP64_MFMA_PEAK_TFLOPS, unit="TFLOP/s",
                        frac=achieved / FP64_MFMA_PEAK_TFLOPS, traffic=traffic)
            if dom == "stht_kernel":
                roof["note"] = "fp64 vector FMAs (the fp64 vector and matrix peaks of gfx950 are the same 78.6 TF); dense-tap flops as the reference computes them"
            if serial_stage:
                roof["serial_stage"] = serial_stage
            roof["traffic_source"] = traffic_src
            if traffic_detail:
                roof["traffic_detail"] = traffic_detail
            roof["algorithmic_bytes_per_launch"] = (frames_launch * C + B * G * 8) if dom == "beamform_kernel" else None  # int8 raster in, power out
            roof["avg_launch_ms"] = st[dom]
            roof["stages_ms"] = st
        names = {"noisy": "target_snn_localization noisy sweep", "speech": "target_snn_localization speech sweep (LibriSpeech 84-121123-0020, per-GPU share of 1000 trials)",
                 "stress": "stress shape (64-mic Random2DArray r=0.2 m after np.random.seed(1), 96 kHz)"}
        result = {
            "metric": "audio samples/sec through STHT+RZCC+SNN beamform, 7-mic 48kHz 360-DoA; DoA MAE vs ref",
            "value": value,
            "unit": "frames/s (one frame = one audio sample instant across all mics)",
            "n_gpus": group_size,
            "rccl_ranks": group_size if (use_dist and not grp.staged) else 0,
            "backend": grp.backend,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "ms_per_step_repeats": [t / args.steps * 1e3 for t in dt_all],
            "ms_per_step_per_rank": ms_per_rank,
            "cpu_cores_per_rank": args.cpu_cores or usable_cores(),
            "timing_note": f"median of {len(dt_all)} timed regions of exactly {args.steps} steps each (barrier + synchronize on both sides, max over ranks), "
                           f"after {settle_steps} settle steps (--settle-seconds {args.settle_seconds:g}) and {args.warmup} warm-up steps",
            "higher_is_better": True,
            "scaling": "strong" if (args.baseline_total and args.config in ("speech", "stress")) else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"{names[args.config]}: {M}-mic, {wl['fs'] // 1000} kHz, T={T}, {B} trials/GPU/step, "
                                   f"{G}-DoA grid, bipolar RZCC, bf_mat designed on device from the 1 s chirp",
                       "trials_per_gpu": B, "frames_per_trial": T, "num_mic": M, "num_doa": G, "mic_samples_per_s": value * M,
                       "parallelism": f"trial-sharded x{group_size}" + (" (REHEARSAL: all ranks time-slice device 0, gloo, host-staged collectives)"
                                                                          if args.share_device else ""),
                       "shared_device": bool(args.share_device), "hip_streams": nstreams, "hip_graphs": not scan_lane,
                       "schedule": (f"scan-lane: eager launches on {nstreams} streams restricted to {32 - scan_lane} compute units per XCD, the "
                                    f"serial checkpoint scans of all batches on one stream that owns the other {scan_lane}") if scan_lane
                                   else "one captured hipGraph per stream, replayed round-robin",
                       "device_uuid_per_rank": uuids,
                       "settle_steps": settle_steps,
                       "memory_gb": memory_gb(device),
                       "design_from_template_seconds": wl["design_seconds"],
                       "design_note": "bf_mat from the 1 s chirp for all G DoAs, entirely on the device (reference: 24.8 s for 449 DoAs on 8 vCPUs, SURVEY 6)"},
            "mae_deg_per_snr": [float(v) for v in (mae * 180 / np.pi).cpu().numpy()],
            # the north star also asks for the fraction of the HBM roofline: algorithmic bytes of the fused sweep
            # (one fp64 frame in, int8 spikes out and back in = 8M + 2M bytes per frame) over the whole job
            "hbm_fraction": {"bytes_per_frame": 10 * M, "achieved_GBs": value / group_size * 10 * M / 1e9, "peak_GBs": HBM_PEAK_GBS,
                             "frac_per_gpu": value / group_size * 10 * M / 1e9 / HBM_PEAK_GBS,
                             "note": "compute-bound path (about 300 flop/B): small by construction, the binding roof is in `roofline` (--full)"},
        }
        if args.full:
            # SURVEY 8d's clock (first kernel of the input side -> results): the same K steps with DoA draw, synthesis and noise
            # regenerated on the device every step, MAE left on the device like `value`
            result["config"].update(value_e2e=e2e["value"], e2e_ms_per_step=e2e["ms_per_step"],
                                    clocks="`value` = hot path on batches resident in HBM (the driver's contract); `config.value_e2e` = input side "
                                           "included (SURVEY 8d)")
            result.update(value_e2e=e2e["value"], e2e=e2e, roofline=roof,
                          variants={"covariance_power": cov_variant, "f32_mfma_beamform": f32_variant})
        if exchange is not None:
            result["exchange"] = exchange
            result["exchange_ms"] = exchange["exchange_ms"]
        if sustained is not None:
            result["sustained"] = sustained
            tw = (sustained.get("telemetry") or {}).get("whole")
            if tw and roof and roof.get("unit") == "TFLOP/s":
                # the datasheet peak assumes the 2.4 GHz boost clock; the chip reports what it actually held during the long region
                pk = FP64_MFMA_PEAK_TFLOPS * tw["sclk_mhz_mean"] / 2400.0
                roof["peak_at_measured_clock"] = pk
                roof["frac_at_measured_clock"] = roof["achieved"] / pk
                roof["measured_clock_mhz"] = tw["sclk_mhz_mean"]
            result["config"]["sustained_ms_per_step"] = sustained["ms_per_step"]
            if sustained["ratio_to_timed_regions"] > 1.02:
                # the long run is more than 2 % slower than the K-step regions (clock / power management): the honest number is the value
                result["value_timed_regions"] = result["value"]
                result["ms_per_step_timed_regions"] = result["ms_per_step"]
                result["value"] = sustained["value"]
                result["ms_per_step"] = sustained["ms_per_step"]
                result["config"]["mic_samples_per_s"] = sustained["value"] * M
                result["value_source"] = (f"sustained region ({sustained['seconds']:.1f} s, {sustained['steps']} steps): the K-step regions were "
                                          f"{(sustained['ratio_to_timed_regions'] - 1) * 100:.1f} % faster than the long run")
                # everything derived from `value` follows it; what still describes the K-step regions says so
                hf = result["hbm_fraction"]
                hf["achieved_GBs"] = sustained["value"] / group_size * hf["bytes_per_frame"] / 1e9
                hf["frac_per_gpu"] = hf["achieved_GBs"] / HBM_PEAK_GBS
                result["timing_note"] = ("`value` / `ms_per_step` = the sustained region (one uninterrupted run, slowest rank); "
                                         "`ms_per_step_repeats` / `ms_per_step_timed_regions` = " + result["timing_note"] +
                                         "; `roofline` times the dominant kernel's launches with HIP events (independent of either clock)")
            else:
                result["value_source"] = (f"median of the K-step regions (the sustained region of {sustained['seconds']:.1f} s agrees within 2 %: "
                                          f"ratio {sustained['ratio_to_timed_regions']:.4f})")
        if args.full and noisy and M * 2 <= 16:
            result["variants"]["beamformer_c128"] = beamformer_c128_block(wl, args)
            result["variants"]["streaming_live"] = streaming_live_block(wl)
        if args.full and noisy and group_size == 1 and not args.no_other_configs:
            torch.cuda.synchronize()
            result["mae_ref"] = reference_mae_block(device)
            result["api_per_call_ms"] = api_per_call_block(device)
            result["other_configs"] = other_configs_block(args)
        if args.full and not args.no_cpu_baseline and group_size == 1 and noisy:
            try:
                cb, am = cpu_baseline(wl, args.cpu_seconds, np_pool, np_workers)
            except Exception as e:  # (a stuck worker pool must not take the line down: the other legs are repeated without it)
                print(f"bench.py: numpy_ops_all_cores leg failed ({type(e).__name__}: {e}); cpu_baseline without it", file=sys.stderr)
                if np_pool is not None:
                    np_pool.terminate()
                    np_pool = None
                cb, am = cpu_baseline(wl, args.cpu_seconds, None, 0)
            am_gpu = argmax_direct.cpu().numpy()
            cb["argmax_equal_to_gpu"] = bool(np.array_equal(am["all"], am_gpu) and np.array_equal(am["one"], am_gpu[: len(am["one"])])
                                             and np.array_equal(am["numpy"], am_gpu[: len(am["numpy"])])
                                             and ("numpy_all" not in am or np.array_equal(am["numpy_all"], am_gpu[: len(am["numpy_all"])])))
            result["cpu_baseline"] = cb
    if np_pool is not None:
        np_pool.terminate()  # (idle workers: nothing to wait for)
        np_pool.join()
    grp.close()
    if rank == 0:
        # RCCL prints a version banner through C stdio on stdout; flush it first so the JSON line is the last line
        import ctypes

        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(result), flush=True)
    return 0


def pin_cpu_cores(n, slot):
    """Restrict this process to `n` of the host cores it may use: slice number `slot` of the allowed set (ranks get disjoint
    slices while they last).  Called before any GPU call, so the HIP runtime's helper threads inherit the mask."""
    allowed = sorted(os.sched_getaffinity(0))
    n = max(1, min(int(n), len(allowed)))
    lo = (slot * n) % max(1, len(allowed) - n + 1)
    os.sched_setaffinity(0, set(allowed[lo : lo + n]))
    return n


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse(argv)
    if args.cpu_cores and "WORLD_SIZE" in os.environ or (args.cpu_cores and args.gpus == 1):
        args.cpu_cores = pin_cpu_cores(args.cpu_cores, int(os.environ.get("LOCAL_RANK", 0)))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # still GPU-free here: nothing above imported torch.cuda state or loaded libmicloc_hip.so
        return launch_ranks(args, argv)
    return run(args)


if __name__ == "__main__":
    sys.exit(main())
