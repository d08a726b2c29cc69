#!/usr/bin/env python3
"""bench.py — PnP solves/second on BASELINE.json's config 2 (1024 proposals x 28x28 correspondences).

    python bench.py --gpus N --steps K --warmup W

With N > 1 and no torch.distributed environment the script starts its own N ranks (one per GPU, RCCL,
rendezvous on 127.0.0.1 — monorun_amd/launch.py, the way /root/reference/train.py:67-74 starts its workers);
started by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` it runs as one of them.

A "step" is one pass of the hot path over one synthetic batch that is already resident in HBM: ONE CALL of the op as the
reference's config dict builds it — the reference's flow: istd mask -> cv2.solvePnPRansac(EPNP, 30 iterations) restated
(five launches one call at a time, six per launch set, + its re-fit's pose candidates as the prologue of the next) -> LM -> covariance (one launch), through the C ABI — over 1024 objects per GPU, plus — when N > 1 — the
single RCCL all-gather of the packed per-object results (north_star: "objects shard across the GPUs with an RCCL all-gather
of poses").  `--flow k0` measures the explicit one-launch fast mode instead (rounds 1-4's `value`); the default line carries
it under `k0_fast_mode`.  Weak scaling: every rank owns 1024 objects per step.  The steps
rotate over --batches DISTINCT resident batches (default 12 x 23.4 MB = 281 MB > the 256 MiB Infinity Cache),
so the inputs really stream from HBM.  W untimed warm-up steps, then EXACTLY K steps between barrier +
torch.cuda.synchronize() pairs; the reported time is the MAX over ranks; rank 0 prints ONE JSON line, the headline (value,
ms_per_step = the wall time of one timed step; with --full also the variants' values and the checks), and with --details FILE writes the whole record
there.  --dump-outputs DIR writes what the last timed step computed (headline key `outputs_dumped`).

A plain run does what the headline needs and no more: it sets up, runs what has always come before the timed window (the validity
check, the same window in the state a just-started process finds the GPU in, the pre-conditioning launches), warms up, times the K
steps, dumps, and prints the line.  `--full` adds everything else after the timed window: the re-check of the timed outputs against
isolated launches, the variants (rotation-normalised, single stream, steady state, grouped collective), the duration of one collective,
the per-launch HIP-event figures and the roofline, the secondary figures, the `--flow k0` child run and the CPU baselines.

Extra objects in the record with --full (prompt ④):
  roofline      dominant kernel's algorithmic bytes / its average launch duration (HIP events around each
                launch, on the stream it is launched on), against the 8 TB/s HBM peak; `flops` = counted fp64
                FLOP per launch (from the kernel's own per-object iteration / inlier counts) against the
                78.6 TFLOP/s fp64 vector peak; `traffic` / `valu_issue` are replayed from profiles/ and say so
  cpu_baseline  the CPU oracle (C restatement of the reference's path, kind "port": the reference's own C++
                needs Ceres and cannot be built here) timed on this box's host cores on a bounded sample of
                the same workload; rank 0, N = 1 only.  Also: the same with the EPnP+RANSAC restatement as the
                initialiser (kind "port+epnp"), and both sides with the initialiser excluded (init_pose given).
  comm          N > 1: backend, number of ranks in the RCCL communicator (ncclCommCount), bytes per rank
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

B_PER_GPU = 1024
HW = 28
P = HW * HW
SEED = 1234
# in = P*(2+2+3)*4 + 36 + 16 + 4 ; out = 16 + 64 + 4 + 1 + P  ->  22 877 B / solve (fp32, P = 784)
BYTES_PER_SOLVE = P * 7 * 4 + 36 + 16 + 4 + 16 + 64 + 4 + 1 + P
LAUNCHES_TEXT = '6 launches per call of fewer than 2048 objects (front, hypotheses, consensus, the second round as ONE launch, re-fit betas, re-fit + LM + covariance), 7 per launch set (the second round as its two compact launches)'
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X_MICROARCH.md: fp64 vector peak (256 CUs x 4 SIMDs x 16 lanes x 2 x 2.4 GHz)
FLOP_PER_POINT_EVAL = 80        # projection ~20, Jacobian ~24, 12 FMA J^T J, 6 FMA J^T r, cost


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=240)
    ap.add_argument('--warmup', type=int, default=24)
    ap.add_argument('--batches', type=int, default=12, help='distinct resident batches the steps rotate over (12 x 23.4 MB > 256 MiB L3)')
    ap.add_argument('--full', action='store_true',
                    help='measure and check everything else after the timed window as well (variants, collective duration, per-launch figures and '
                         'roofline, output re-check, secondary figures, the --flow k0 child run, CPU baselines); a plain run times the headline only')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baselines')
    ap.add_argument('--no-secondary', action='store_true', help='with --full: skip the secondary figures (multi-stream, 8192-object launch, per-image latency)')
    ap.add_argument('--cpu-seconds', type=float, default=20.0, help='with --full: target CPU-baseline sample time (all legs together)')
    ap.add_argument('--waves', type=int, default=0, help='wavefronts per object (0 = library heuristic)')
    ap.add_argument('--in-flight', type=int, default=int(os.environ.get('MR_BENCH_IN_FLIGHT', '4')),
                    help='launches in flight: the steps are issued round-robin on this many HIP streams through monorun_amd.PnPPipeline '
                         '(1 = one stream, every launch waits for the previous one; reported as single_stream either way)')
    ap.add_argument('--flow', choices=['reference', 'k0'], default=os.environ.get('MR_BENCH_FLOW', 'reference'),
                    help="reference (default): what the drop-in boundary runs — the reference's flow, cv2.solvePnPRansac(EPNP, 30) restated on the GPU + LM "
                         "+ covariance (PnPUncert built from the reference's config dict); k0: the explicit one-launch fast mode (PnPUncert(initialiser='k0')), "
                         'what rounds 1-4 reported as `value`.  With --flow reference the line carries the fast mode under `k0_fast_mode`')
    ap.add_argument('--group', type=int, default=int(os.environ.get('MR_BENCH_GROUP', '5')),
                    help='reference flow, launches in flight: calls whose initialiser launches are issued as ONE launch set (monorun_amd.PnPEpnpGroupLaunch, '
                         '1..8; every call keeps its own inputs and outputs)')
    ap.add_argument('--workload', choices=['config2', 'stress'], default='config2',
                    help="config2 (default, the metric's configuration) or stress = BASELINE config 5's per-GPU shard: 8192 objects x "
                         '56x56 correspondences, fp16 storage (a parity-test shape; an extra line, never the judged one)')
    ap.add_argument('--details', metavar='FILE', default=None,
                    help='write the whole record (configuration, rooflines, variants, secondary figures, CPU baselines) to FILE as one JSON '
                         'line; stdout carries the headline line only')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step computed — the launch outputs a caller receives: valid, pose, cov, '
                         'tr, inlier_mask (+ all_ranks_* from the all-gather when N > 1) — as DIR/<name>.npy in float32, at most 64 MB in all '
                         '(beyond that a fixed seeded sample of inlier_mask rows, their indices in inlier_mask_rows.npy as float64).  Same arguments, same inputs: '
                         'two builds can be compared output for output')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


def host_threads():
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:                                               # containers: honour the cgroup CPU quota (e.g. "1600000 100000" = 16 cores)
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()
        if q != 'max':
            n = max(1, min(n, int(int(q) / int(per))))
    except Exception:  # noqa: BLE001
        pass
    return n


def perturbed_gt_init(batch, seed):
    """Initial poses for the initialiser-excluded figures: ground truth + a seeded perturbation
    (sigma 0.1 rad, 0.3 m, 0.1 m, 1.0 m) — identical on the GPU and CPU side."""
    rng = np.random.default_rng(seed)
    gt = np.concatenate([batch['gt_yaw'][:, None], batch['gt_t']], 1)
    return gt + rng.normal(0.0, 1.0, gt.shape) * np.array([0.1, 0.3, 0.1, 1.0])


DUMP_LIMIT_BYTES = 64_000_000


def write_outputs(dirname, arrays, seed=SEED):
    """--dump-outputs: arrays (name -> numpy array) as DIR/<name>.npy, float64 kept, everything else as float32.  If they exceed
    DUMP_LIMIT_BYTES together, the largest one (the inlier masks of a large workload) is cut to a fixed seeded sample of its rows
    and <name>_rows.npy holds their indices.  Returns the names written."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.asarray(v, np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        big = max(arrays, key=lambda k: arrays[k].nbytes)
        a = arrays[big]
        row = a.nbytes // a.shape[0]
        k = (DUMP_LIMIT_BYTES - 64 * 1024 - (total - a.nbytes)) // (row + 8)         # 64 KiB left for the .npy headers
        rows = np.sort(np.random.default_rng(seed).choice(a.shape[0], k, replace=False))
        arrays[big], arrays[big + '_rows'] = a[rows], rows.astype(np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + '.npy'), a)
    return sorted(arrays)


def cpu_baseline(np_inputs, init_pose, seconds, ref_flow=True, workload='config-2 batch 0'):
    """The oracle (C restatement, fp64, -O2 like the reference) on a bounded sample of the same workload.
    1 thread = the reference's execution model (serial multi_apply, Ceres num_threads=1); all cores = fair ceiling.
    `cpu_baseline` is the flow `value` was measured on: the reference's own (EPnP inside OpenCV's RANSAC loop, pnp_uncert_cpu.py:35-58,
    restated; then the LM) with --flow reference, the K0 specification with --flow k0; the other flow rides along."""
    from oracle import oracle as orc
    x2d, istd, x3d, K, ur, vr, thr = np_inputs
    out = {}
    big = x2d.shape[1] > 1024                          # stress shape: 3136 points per object

    def timed(fn, n_obj, budget, max_reps=200):
        t0 = time.perf_counter()
        reps = 0
        while True:
            fn()
            reps += 1
            el = time.perf_counter() - t0
            if el >= budget or reps >= max_reps:
                return n_obj * reps / el, reps, el
    flows = {'epnp': (orc.u2d_pnp_epnp, 'EPnP + RANSAC restatement (30 iterations, 5-point samples) — the reference\'s initialiser', 'port+epnp', 32 if big else 128),
             'k0': (orc.u2d_pnp, 'K0 (this repo\'s consensus initialiser)', 'port', 64 if big else 256)}
    main, other = ('epnp', 'k0') if ref_flow else ('k0', 'epnp')
    fn, name, kind, n1 = flows[main]
    n1 = min(n1, x2d.shape[0])
    v, reps, el = timed(lambda: fn(x2d[:n1], istd[:n1], x3d[:n1], K, ur, vr, 0.5, 0.6, thr[:n1], True, num_threads=1), n1, seconds * 0.35)
    out['cpu_baseline'] = dict(value=v, unit='solves/s', cores=1, kind=kind, initialiser=name,
                               sample=f'first {n1} objects of {workload} x {reps} repeats, {el:.1f} s, single thread '
                                      '(the reference runs objects serially with Ceres num_threads=1)')
    nthr = host_threads()
    nall = min(x2d.shape[0], 256 if big else x2d.shape[0])
    v, reps, el = timed(lambda: fn(x2d[:nall], istd[:nall], x3d[:nall], K, ur, vr, 0.5, 0.6, thr[:nall], True, num_threads=nthr), nall, seconds * 0.2)
    out['cpu_baseline_all_cores'] = dict(value=v, unit='solves/s', cores=nthr, kind=kind, initialiser=name,
                                         sample=f'first {nall} objects of {workload} x {reps} repeats, {el:.1f} s, OpenMP over objects')
    fn2, name2, kind2, n2 = flows[other]
    n2 = min(n2, x2d.shape[0])
    v, reps, el = timed(lambda: fn2(x2d[:n2], istd[:n2], x3d[:n2], K, ur, vr, 0.5, 0.6, thr[:n2], True, num_threads=1), n2, seconds * 0.3)
    out['cpu_baseline_' + other] = dict(value=v, unit='solves/s', cores=1, kind=kind2, initialiser=name2,
                                        sample=f'first {n2} objects of {workload} x {reps} repeats, {el:.1f} s, single thread')
    out['cpu_baseline_' + main] = out['cpu_baseline']
    if init_pose is not None:
        n3 = min(64 if big else 256, x2d.shape[0])
        v, reps, el = timed(lambda: orc.u2d_pnp(x2d[:n3], istd[:n3], x3d[:n3], K, ur, vr, 0.5, 0.6, thr[:n3], True, init_pose=init_pose[:n3], num_threads=1),
                            n3, seconds * 0.15)
        out['cpu_baseline_init_given'] = dict(value=v, unit='solves/s', cores=1, kind='port', initialiser='none (init_pose = GT + seeded perturbation)',
                                              sample=f'first {n3} objects x {reps} repeats, {el:.1f} s, single thread; istd mask + LM + covariance only')
    return out


def main():
    args = parse()
    from monorun_amd import launch
    if args.gpus > 1 and not launch.in_distributed_job():
        # self-launch: one rank per GPU.  MR_BENCH_OVERSUBSCRIBE=1 (test mode) allows more ranks than devices; RCCL refuses
        # two ranks on one device, so that mode exchanges through gloo and says so in the `comm` block.
        oversub = os.environ.get('MR_BENCH_OVERSUBSCRIBE') == '1'
        sys.exit(launch.spawn_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:], need_devices=not oversub))
    run(args)


_JSON_FD = None


def _protect_stdout():
    """The contract is ONE JSON line on stdout.  Native libraries print there too (RCCL's version banner, ROCm warnings), and their
    C-level buffers are flushed at exit, i.e. after the line: everything written to fd 1 from here on goes to stderr, and the line
    itself is written to the saved descriptor."""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


HEADLINE_KEYS = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data',
                 'value_cold', 'value_rotation_normalised', 'valid_fraction', 'outputs_verified', 'speedup_vs_cpu_1thread', 'speedup_vs_cpu_all_cores',
                 'comm', 'outputs_dumped')


def headline(line):
    """The result line printed on stdout.  The whole record is ~20 KB, more than a log that keeps the end of a run's output holds, so the
    line carries the headline figures (a few hundred bytes) and --details FILE the record."""
    h = {k: line[k] for k in HEADLINE_KEYS if k in line}
    h['flow'] = line['config']['flow'].split(':')[0]
    for k in ('steady_state', 'single_stream', 'k0_fast_mode', 'cpu_baseline'):
        if isinstance(line.get(k), dict) and 'value' in line[k]:
            h['value_' + k] = line[k]['value']
    return h


def _emit(line):
    data = (json.dumps(line) + '\n').encode()
    if _JSON_FD is None:
        sys.stdout.write(data.decode()); sys.stdout.flush()
    else:
        os.write(_JSON_FD, data)


def run(args):
    _protect_stdout()
    global B_PER_GPU, HW, P, SEED, BYTES_PER_SOLVE
    import torch
    import torch.distributed as dist
    from monorun_amd import synthetic as syn
    from monorun_amd import PnPLaunch, PnPEpnpLaunch, PnPEpnpGroupLaunch, PnPPipeline
    from monorun_amd.parallel import PackedResults, ROW_BYTES

    stress = args.workload == 'stress'
    ref_flow = args.flow == 'reference'
    if stress:                                   # 47 181 B / solve (fp16, P = 3136)
        B_PER_GPU, HW, SEED = 8192, 56, 4321
        P = HW * HW
        BYTES_PER_SOLVE = P * 7 * 2 + 36 + 16 + 4 + 16 + 64 + 4 + 1 + P
        args.no_secondary = True
        args.batches = 1                         # one 8192-object fp16 batch is 360 MB: already larger than the Infinity Cache
        args.in_flight = 1                       # an 8192-object launch fills the chip by itself
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit(f'bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; start it as `python bench.py --gpus N` '
                         '(it launches its own ranks) or through torch.distributed.run with --nproc-per-node N')
    assert torch.cuda.is_available(), 'bench.py needs an MI355X (no CPU fallback)'
    ndev = torch.cuda.device_count()
    oversub = os.environ.get('MR_BENCH_OVERSUBSCRIBE') == '1' and world > ndev
    if world > ndev and not oversub:
        raise SystemExit(f'bench.py: {world} ranks but only {ndev} visible MI355X devices (one rank per GPU over RCCL)')
    torch.cuda.set_device(local_rank % ndev)
    dev = torch.device('cuda', local_rank % ndev)
    # MR_BENCH_FORCE_DIST=1 runs the RCCL path (init, all-gather, barrier, max-reduce) even at world size 1 — the only way
    # to exercise it on a 1-GPU box
    use_dist = world > 1 or os.environ.get('MR_BENCH_FORCE_DIST') == '1'
    if use_dist:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        if oversub:
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    def to_dev(a):
        t = torch.from_numpy(np.asarray(a))
        d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=dev)
        d.copy_(t)
        return d

    # ---- synthetic batches, resident in HBM.  Batch 0 is the config's own seed.  Every rank holds the SAME NB batches and walks them
    #      with a rank-dependent offset: at any step the ranks solve different batches (weak scaling: N x 1024 distinct objects per
    #      step while NB >= N), but over a full rotation every rank does the same work — a launch lasts as long as its slowest object
    #      (56 - 98 us between batches), and with per-rank seeds the N-GPU figure would measure which rank drew the slowest batches,
    #      not how the system scales.
    NB = max(1, args.batches)
    seeds = [SEED + 7919 * i for i in range(NB)]
    rot0 = (rank * NB) // max(world, 1)                      # this rank's starting offset into the rotation
    dev_batches, np_batch0, batch0 = [], None, None
    for i, sd in enumerate(seeds):
        if stress:                               # 1024 distinct objects, tiled 8x (generation time), stored as fp16 channel-planar
            batch = syn.make_batch(B=1024, hw=HW, seed=sd)
            np_inputs = syn.pnp_boundary(batch, planar=True)
            rep8 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).transpose(0, 2, 1))).to(dev).to(torch.float16).repeat(8, 1, 1).permute(0, 2, 1)
            x2d, istd, x3d = [rep8(a) for a in np_inputs[:3]]
            K, ur, vr = [to_dev(a) for a in np_inputs[3:6]]
            thr = to_dev(np_inputs[6]).repeat(8)
        else:
            batch = syn.make_batch(B=B_PER_GPU, hw=HW, seed=sd)
            np_inputs = syn.pnp_boundary(batch, planar=True)     # the strided views the reference's head hands to the PnP
            x2d, istd, x3d, K, ur, vr, thr = [to_dev(a) for a in np_inputs]
        dev_batches.append((x2d, istd, x3d, K, ur, vr, thr))
        if i == 0:
            np_batch0, batch0 = [np.asarray(a) for a in np_inputs], batch
    resident_bytes = sum(sum(t.numel() * t.element_size() for t in b[:3]) for b in dev_batches)

    # exchange: a private RCCL communicator driven directly (ncclAllGather on a high-priority side stream, ~5 us of host time per
    # call); MR_BENCH_COMM=torch, or any failure to set it up, falls back to torch.distributed's (synchronous) all-gather
    rccl, rccl_why = None, None
    if use_dist and not oversub and os.environ.get('MR_BENCH_COMM', 'rccl') == 'rccl':
        # every rank or none (a rank that cannot build its private communicator must not leave the others inside a collective): any
        # set-up problem on any rank drops the whole job to torch.distributed's all-gather, and the `comm` block says why
        from monorun_amd.parallel import agreed_rccl_all_gather
        rccl, rccl_why = agreed_rccl_all_gather(dev)
        if rccl is None:
            print(f'[bench] rank {rank}: direct RCCL path unavailable ({rccl_why}); the job uses torch.distributed\'s all-gather', file=sys.stderr)
    # Launches in flight.  One launch of 1024 objects lasts as long as its slowest object, and launches on one stream serialise;
    # the product's PnPPipeline issues the steps round-robin on L streams so that the next batches fill the SIMDs a launch's tail
    # leaves idle.  Every step is still ONE full config-2 launch over its own batch into its own result buffers.
    pipes = {}

    def pipe_of(depth):
        if depth not in pipes:      # the streams are picked by measurement: mutually overlapping, and not on the exchange's queue
            pipes[depth] = PnPPipeline(dev, depth=depth, avoid=[rccl.stream] if rccl is not None else ())
        return pipes[depth]
    L_ASKED = max(1, args.in_flight)
    L = pipe_of(L_ASKED).depth                         # launches really in flight (streams found to run side by side)
    # Result buffers: S slots (packed 88 B/object rows + inlier masks), slot s pinned to pipeline stream s % L.  With N > 1 every
    # step's packed rows are exchanged by ONE all-gather (north_star: "RCCL all-gather of poses"; G = 1 by default) on the side
    # stream, behind that step's completion event, while the following steps compute.  MR_BENCH_GATHER_EVERY=G groups G
    # consecutive steps (one contiguous G x 88 KiB buffer) into one collective: measured as secondary_throughput.grouped_collective.
    G_SEC = 8
    RING = max(2, int(os.environ.get('MR_BENCH_RING', '4')))
    S = RING * G_SEC                                   # 32 slots: multiple of every L <= 8 and of G_SEC
    LG = max(1, min(8, args.group)) if (ref_flow and L > 1 and not stress and not oversub) else 1      # calls per launch set (reference flow)
    while S % L or S % LG:
        S += G_SEC
    row = B_PER_GPU * ROW_BYTES
    gbuf = [torch.zeros(G_SEC * row, dtype=torch.uint8, device=dev) for _ in range(S // G_SEC)]
    packs = [PackedResults(B_PER_GPU, dev, buf=gbuf[sl // G_SEC][(sl % G_SEC) * row:(sl % G_SEC + 1) * row]) for sl in range(S)]
    masks = [torch.empty(B_PER_GPU, P, device=dev, dtype=torch.uint8) for _ in range(S)]

    # waves per object: --waves, else the pipeline's rule (the library's own rule applied to the objects of all launches in flight)
    fl_main = (args.waves << 8) if args.waves else pipe_of(L_ASKED).flags_for(B_PER_GPU, P)
    fl_one = (args.waves << 8)                              # one launch at a time: the library's heuristic

    # reference flow: the initialiser's launches hand their intermediate results over in a workspace — one per result slot (a slot is
    # pinned to one pipeline stream, so its launches are stream-ordered), shared by every batch's launch object of that slot; a launch
    # GROUP (calls of consecutive slots issued as one launch set) uses the group's first slot's, sized for the whole group
    works = None
    if ref_flow:
        from monorun_amd import _lib as _mrlib
        wbytes = int(_mrlib.load().mr_epnp_workspace_bytes(B_PER_GPU * LG, P))
        works = [torch.empty(wbytes if (LG == 1 or k % LG == 0) else int(_mrlib.load().mr_epnp_workspace_bytes(B_PER_GPU, P)), device=dev, dtype=torch.uint8) for k in range(S)]

    def mk(bi, k, flags=None, **kw):
        x2d, istd, x3d, K, ur, vr, thr = dev_batches[bi]
        if ref_flow:
            return PnPEpnpLaunch(x2d, istd, x3d, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr, inlier_opt_only=True,
                                 flags=fl_main if flags is None else flags, out=packs[k] if k is not None else None, mask=masks[k] if k is not None else None,
                                 work=works[k] if k is not None else None, **kw)
        return PnPLaunch(x2d, istd, x3d, K, ur, vr, z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=thr, inlier_opt_only=True,
                         flags=fl_main if flags is None else flags, out=packs[k] if k is not None else None, mask=masks[k] if k is not None else None, **kw)
    launches = [[mk(bi, k) for k in range(S)] for bi in range(NB)]
    group_cache = {}

    def group_of(table, bi0, sl0, n):
        """The launch set of the n calls (batch bi0 + j, slot sl0 + j): built on first use (ctypes pointer tables only; the members own the buffers)."""
        key = (id(table), bi0, sl0, n)
        if key not in group_cache:
            group_cache[key] = PnPEpnpGroupLaunch([table[(bi0 + j) % NB][sl0 + j] for j in range(n)], work=works[sl0])
        return group_cache[key]
    launches_one = launches if fl_one == fl_main else [[mk(bi, k, flags=fl_one) for k in range(S)] for bi in range(NB)]
    gathered_step = [torch.empty(world * row, dtype=torch.uint8, device=dev) for _ in range(S)] if use_dist else None
    gathered_grp = [torch.empty(world * b.numel(), dtype=torch.uint8, device=dev) for b in gbuf] if use_dist else None
    if use_dist and oversub:
        host_send = torch.empty(row, dtype=torch.uint8).pin_memory()
        host_recv = torch.empty(world * row, dtype=torch.uint8).pin_memory()
    class Loop:
        """K steps of the hot path: launch (+ exchange).  depth = launches in flight, G = steps per collective."""

        def __init__(self, depth, G):
            self.depth, self.G = depth, (G if rccl is not None else 1)
            self.pipe = pipe_of(L_ASKED if depth == L else depth)
            self.launches = launches if depth == L else launches_one
            self.done = [None] * S          # completion event of the collective that last READ slot s (or its group)
            self.evs = [None] * S           # completion event of the launch that last WROTE slot s
            self.i = 0
            self.lg = LG if depth > 1 else 1        # calls per launch set (reference flow in flight); one call at a time is never grouped
            self.pend = []                  # (batch, slot) of the calls of the launch set being collected

        def _before(self, sl):
            """What must have happened before slot sl is rewritten: its previous exchange (S steps ago) has finished."""
            if not use_dist or oversub or rccl is None:
                return
            G = self.G
            g0 = sl - sl % G                                        # first slot of this step's group
            d = self.done[g0]
            if d is not None and sl == g0:
                # the group is about to be rewritten: its previous exchange must have finished; normally it has, long ago
                if not d.query():
                    for st in self.pipe.streams:
                        st.wait_event(d)
                self.done[g0] = None

        def _after(self, sl):
            """The exchange of slot sl's packed rows, behind the completion event of the launch (set) that wrote them."""
            if not use_dist:
                return
            if oversub:
                self.evs[sl].synchronize()
                host_send.copy_(packs[sl].buf)
                dist.all_gather_into_tensor(host_recv, host_send)
                gathered_step[sl].copy_(host_recv, non_blocking=True)
                return
            if rccl is None:
                torch.cuda.current_stream().wait_event(self.evs[sl])
                dist.all_gather_into_tensor(gathered_step[sl], packs[sl].buf)
                return
            G = self.G
            if sl % G == G - 1:
                self.exchange(sl - sl % G, sl)

        def flush(self):
            """Issue the calls collected so far as one launch set on the stream of the set's first slot, then their exchanges."""
            if not self.pend:
                return
            bi0, sl0 = self.pend[0]
            n = len(self.pend)
            pend, self.pend = self.pend, []
            if n > 1 and sl0 % self.lg == 0:
                ev = self.pipe.submit(group_of(self.launches, bi0, sl0, n), slot=sl0 // self.lg)
                for _, sl in pend:
                    self.evs[sl] = ev
            else:
                # one call, or a set that does not start on a set boundary (stepping went on after a fence in the middle of a set: only the
                # workspace of a set's FIRST slot is sized for a whole set): the calls one by one, each with its own slot's
                # workspace, on the stream their set would have used
                for bi, sl in pend:
                    self.evs[sl] = self.pipe.submit(self.launches[bi][sl], slot=sl // self.lg if self.lg > 1 else sl)
            for _, sl in pend:
                self._after(sl)

        def step(self):
            i = self.i
            self.i += 1
            bi = (i + rot0) % NB
            sl = i % S
            self._before(sl)
            # reference flow with launches in flight: consecutive steps (consecutive slots, aligned to the group size) form one launch
            # set; otherwise every step is its own launch (set)
            self.pend.append((bi, sl))
            if self.lg == 1 or sl % self.lg == self.lg - 1 or sl == S - 1:
                self.flush()

        def exchange(self, g0, last):
            G = self.G
            if G == 1:
                self.done[g0] = rccl.gather(packs[last].buf, gathered_step[last], after=self.evs[last])
                return
            # the group's steps ran on several streams: the collective waits for every launch (set) of the group
            seen = set()
            for sl in range(g0, last):
                if self.evs[sl] is not None and id(self.evs[sl]) not in seen:
                    seen.add(id(self.evs[sl]))
                    rccl.stream.wait_event(self.evs[sl])
            gi = g0 // G_SEC
            nb = (last - g0 + 1) * row                               # a partly filled group at the fence: what there is
            send = gbuf[gi] if nb == gbuf[gi].numel() else gbuf[gi][:nb]
            recv = gathered_grp[gi] if nb == gbuf[gi].numel() else gathered_grp[gi][:world * nb]
            self.done[g0] = rccl.gather(send, recv, after=self.evs[last])

        def fence(self):
            self.flush()
            if use_dist and rccl is not None and self.G > 1 and self.i % self.G != 0:
                last = (self.i - 1) % S
                self.exchange(last - last % self.G, last)
            self.pipe.drain()
            if use_dist:
                if rccl is not None:
                    rccl.stream.synchronize()
                torch.cuda.synchronize()
                dist.barrier()
            torch.cuda.synchronize()

        def timed(self, steps, warmup):
            for _ in range(warmup):
                self.step()
            self.fence()
            self.i = 0                                               # the timed window starts at rotation offset 0 (+ the rank's offset)
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step()
            t_issue = time.perf_counter() - t0
            self.fence()
            el = time.perf_counter() - t0
            if os.environ.get('MR_BENCH_DEBUG'):
                print(f'[bench] depth {self.depth} G {self.G}: {steps} steps issued in {t_issue * 1e6:.0f} us ({t_issue / steps * 1e6:.1f} us/step), complete after {el * 1e6:.0f} us', file=sys.stderr)
            if use_dist:
                t = torch.tensor([el], dtype=torch.float64, device='cpu' if oversub else dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el = float(t.item())
            return el

    G_MAIN = max(1, int(os.environ.get('MR_BENCH_GATHER_EVERY', '1')))
    if G_MAIN not in (1, G_SEC):
        G_MAIN = 1
    def diagnose():
        """Per-object diagnostics of every batch (LM iterations, final inlier counts): the validity check + the FLOP count."""
        valid_n, flop_total, it_hist = 0, 0.0, {}
        for bi in range(NB):
            ld = mk(bi, None, with_diag=True)
            ld.run()
            torch.cuda.synchronize()
            valid_n += int(ld.valid.sum().item())
            iters = ld.diag[:, 0].double()
            n_inl = ld.mask.sum(1).double()
            # LM: (iterations + 1) evaluations of the inlier set (cost + J^T J + J^T r), + 1 covariance pass
            flop_total += float((FLOP_PER_POINT_EVAL * n_inl * (iters + 2)).sum().item())
            for v, c in zip(*np.unique(iters.cpu().numpy().astype(int), return_counts=True)):
                it_hist[int(v)] = it_hist.get(int(v), 0) + int(c)
        valid_frac = valid_n / float(NB * B_PER_GPU)
        assert valid_frac > 0.95, f'only {valid_frac:.3f} of the solves are valid — refusing to report a number'
        return valid_frac, flop_total / NB, it_hist

    # the validity check runs BEFORE the timed window (a bench that is going to refuse should refuse before it measures); measured
    # side effect: the GPU has seen 12 launches when the warm-up starts, worth ~2 % on the driver's 20-step window (31.3 -> 32.0 M,
    # 6 processes each way, profiles/r03_bench_order.txt).  MR_BENCH_DIAG_FIRST=0 puts it back after the measurements.
    diag_first = os.environ.get('MR_BENCH_DIAG_FIRST', '1') == '1'
    if diag_first:
        valid_frac, flops_per_launch, it_hist = diagnose()
    # Device pre-conditioning, untimed and reported (config.prewarm): a process that has just started finds the GPU in its idle power
    # state, and the driver's 20-step window (~0.6 ms) is over before the clocks have come up — measured: the same window is 8 - 9 %
    # slower in a fresh process than after ~40 ms of launches (profiles/r04_closing_schedule_experiment.txt).  A serving process is
    # never in that state, so MR_BENCH_PREWARM_LAUNCHES (default 2048, ~ 60 ms) launches of the hot path are issued through the same
    # pipeline first; the W warm-up steps of the contract follow as before.
    # (a FIXED count per flow and workload — every rank issues the same launches —: ~0.1 s of them)
    prewarm_n = int(os.environ.get('MR_BENCH_PREWARM_LAUNCHES', '64' if stress else ('768' if ref_flow else '2048')))
    prewarm = {'launches_asked': prewarm_n, 'launches': 0, 'ms': 0.0}
    if prewarm_n > 0:
        # the same K-step window first, as a just-started process sees it (reported beside `value`, never as `value`)
        cold = Loop(L, G_MAIN).timed(args.steps, args.warmup)
        prewarm['window_before'] = {'steps': args.steps, 'warmup': args.warmup, 'value': B_PER_GPU * world * args.steps / cold, 'unit': 'solves/s',
                                    'what': 'the timed window as measured BEFORE the pre-conditioning (idle clocks), same loop, same steps'}
        # at most prewarm_n launches and about 0.1 s of them (a stress-shape launch lasts ~ 1 ms), no collective in here, through the
        # pipeline of the timed loop
        pp = pipe_of(L_ASKED)
        t0 = time.perf_counter()
        for blk in range((prewarm_n + S - 1) // S):
            for sl in range(S):
                pp.submit(launches[(blk * S + sl) % NB][sl], slot=sl)
            pp.drain()
            prewarm['launches'] += S
        torch.cuda.synchronize()
        prewarm['ms'] = (time.perf_counter() - t0) * 1e3
    main_loop = Loop(L, G_MAIN)
    elapsed = main_loop.timed(args.steps, args.warmup)
    gather_ok = None
    if use_dist and args.full:                   # the gathered buffer holds every rank's rows (rank-major): check this rank's slice
        torch.cuda.synchronize()
        sl = (main_loop.i - 1) % S
        if main_loop.G == 1:
            gather_ok = bool(torch.equal(gathered_step[sl][rank * row:(rank + 1) * row], packs[sl].buf))
        else:
            gi = sl // G_SEC
            nb = (sl % G_SEC + 1) * row
            gather_ok = bool(torch.equal(gathered_grp[gi][rank * nb:(rank + 1) * nb], gbuf[gi][:nb]))
    # --dump-outputs: the last timed step's own result slot, copied now (the loops below reuse the slots)
    dumped = None
    if args.dump_outputs and rank == 0:
        torch.cuda.synchronize()
        sl = (main_loop.i - 1) % S
        out = {'valid': packs[sl].valid, 'pose': packs[sl].pose, 'cov': packs[sl].cov, 'tr': packs[sl].tr, 'inlier_mask': masks[sl]}
        if use_dist:                             # what every rank receives: the gathered rows of all ranks for this step (rank-major)
            if main_loop.G == 1:
                flat = gathered_step[sl].view(world, row)
            else:
                nb = (sl % G_SEC + 1) * row
                flat = gathered_grp[sl // G_SEC][:world * nb].view(world, nb)[:, nb - row:]
            out.update({'all_ranks_' + k: v for k, v in PackedResults.unpack(flat, world * B_PER_GPU).items()})
        names = write_outputs(args.dump_outputs, {k: v.cpu().numpy() for k, v in out.items()})
        dumped = {'dir': args.dump_outputs, 'files': [n + '.npy' for n in names], 'step': main_loop.i - 1,
                  'batch_seed': seeds[(main_loop.i - 1 + rot0) % NB], 'flags': fl_main}
    outputs_ok, variants = None, {}
    if args.full:
        # every slot written inside the timed window holds exactly what an isolated launch of the same batch produces
        outputs_ok = True
        for i in range(max(0, main_loop.i - S), main_loop.i):
            bi, sl = (i + rot0) % NB, i % S
            ref = (PnPEpnpLaunch if ref_flow else PnPLaunch)(*dev_batches[bi][:6], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=dev_batches[bi][6], inlier_opt_only=True, flags=fl_main)
            ref.run()
            torch.cuda.synchronize()
            outputs_ok = outputs_ok and bool(torch.equal(ref.pose, packs[sl].pose) and torch.equal(ref.cov, packs[sl].cov) and
                                             torch.equal(ref.valid, packs[sl].valid) and torch.equal(ref.mask, masks[sl]))
        assert outputs_ok, 'a pipelined (grouped) launch produced results that differ from an isolated launch of the same batch'
        # the same loop over a whole number of rotations (the driver's --steps need not be a multiple of --batches, and the batches
        # take 56 - 98 us each), and on ONE stream (every launch waits for the previous one: what rounds 1 and 2 reported as `value`)
        rot_steps = ((args.steps + NB - 1) // NB) * NB
        variants['rotation_normalised'] = {'steps': rot_steps, 'elapsed': Loop(L, G_MAIN).timed(rot_steps, min(args.warmup, NB))}
        if L != 1:
            variants['single_stream'] = {'steps': rot_steps, 'elapsed': Loop(1, G_MAIN).timed(rot_steps, min(args.warmup, NB))}
        if use_dist and rccl is not None:
            variants['grouped_collective'] = {'steps': rot_steps, 'elapsed': Loop(L, G_SEC if G_MAIN == 1 else 1).timed(rot_steps, min(args.warmup, NB)),
                                              'steps_per_collective': G_SEC if G_MAIN == 1 else 1}
        # steady state: the same loop over >= 240 steps (the driver's 20-step window carries ~10 % of pipeline fill and drain)
        ss_steps = ((max(240, args.steps) + NB - 1) // NB) * NB
        variants['steady_state'] = {'steps': ss_steps, 'elapsed': Loop(L, G_MAIN).timed(ss_steps, min(args.warmup, NB))}
    comm = None
    if use_dist and oversub:
        comm = {'backend': 'gloo (host-staged; MR_BENCH_OVERSUBSCRIBE test mode: several ranks share one GPU, which RCCL refuses)',
                'nranks': dist.get_world_size(), 'bytes_per_rank': row, 'steps_per_collective': 1}
    elif use_dist:
        comm = {'backend': 'rccl (private communicator, ncclAllGather on a side stream behind the step\'s completion event, overlapped with the following steps)' if rccl is not None
                else ('rccl via torch.distributed (nccl backend) all_gather_into_tensor' +
                      (f' — FALLBACK: the private RCCL communicator could not be set up on every rank ({rccl_why}); ~45 us of host time per collective instead of ~5' if rccl_why else '')),
                'nranks': rccl.nranks() if rccl is not None else dist.get_world_size(),
                'bytes_per_rank': main_loop.G * row, 'steps_per_collective': main_loop.G, 'result_slots': S}
        if rccl is not None and args.full:
            # duration of the collective itself: timing events on the side stream around isolated all-gathers of one step's rows
            e0 = [torch.cuda.Event(enable_timing=True) for _ in range(20)]
            e1 = [torch.cuda.Event(enable_timing=True) for _ in range(20)]
            torch.cuda.synchronize(); dist.barrier()
            for k in range(20):
                e0[k].record(rccl.stream)
                rccl.lib.ncclAllGather(packs[0].buf.data_ptr(), gathered_step[0].data_ptr(), row, rccl.NCCL_UINT8, rccl.comm, rccl.stream.cuda_stream)
                e1[k].record(rccl.stream)
            rccl.stream.synchronize()
            us = float(np.median([a.elapsed_time(b) for a, b in zip(e0[5:], e1[5:])])) * 1e3
            comm['us_per_collective'] = us
            comm['algbw_GBps'] = world * row / (us * 1e-6) / 1e9
            comm['algbw_definition'] = 'bytes every rank ends up with (nranks x bytes_per_rank at 1 step per collective) / median duration of an isolated collective'
    main_loop = None

    k_fl_ms = None
    if args.full:
        # dominant-kernel duration: HIP events around each launch on the launch stream (torch's current stream), rotating batches
        n_ev = min(max(args.steps, NB), 240)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_ev)]
        torch.cuda.synchronize()
        for i in range(3):                                  # untimed: the first launches after an idle period run at reduced clocks (2 x the time), which a
            launches_one[(NB - 3 + i) % NB][0].run()        # 20-launch average would carry; the rocprofv3 average this figure is checked against has hundreds
        for i, (e0, e1) in enumerate(evs):
            e0.record()
            launches_one[i % NB][0].run()
            e1.record()
        torch.cuda.synchronize()
        k_ms = np.array([e0.elapsed_time(e1) for e0, e1 in evs])
        kernel_ms = float(k_ms.mean())
        per_batch_ms = [float(k_ms[bi::NB].mean()) for bi in range(NB)]

        # ... and of the timed regime's own launches: HIP events on the PIPELINE's streams (the streams these kernels are launched on)
        # around every launch of a 240-step run of the timed loop's issue pattern.  The launches overlap, so this is the time a launch is
        # resident, not what it costs the chip: the chip-level rate is value x bytes.
        if L > 1 and not use_dist and not ref_flow:
            pp = pipe_of(L_ASKED)
            nfl = 240
            fev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(nfl)]
            for i in range(2 * L):
                pp.submit(launches[i % NB][i % S], slot=i % S)
            pp.drain()
            for i, (e0, e1) in enumerate(fev):
                st = pp.streams[(i % S) % pp.depth]
                e0.record(st)
                launches[i % NB][i % S].run(pp.handles[(i % S) % pp.depth])
                e1.record(st)
            pp.drain()
            k_fl_ms = np.array([e0.elapsed_time(e1) for e0, e1 in fev])

    if not diag_first:
        valid_frac, flops_per_launch, it_hist = diagnose()

    extra = {}
    if args.full and world == 1 and not args.no_secondary and not ref_flow:
        extra = secondary(args, torch, syn, PnPLaunch, dev, dev_batches, batch0, np_batch0, NB)
    if args.full and ref_flow and world == 1 and not args.no_secondary and not stress:
        try:
            extra['head_to_pose_1024_reference_flow'] = head_to_pose_reference(torch, syn, dev)
        except Exception as e:                                          # noqa: BLE001 — secondary figure
            extra['head_to_pose_1024_reference_flow'] = {'error': repr(e)}
        # the regime the pipeline runs (one image, <= 100 proposals, one call at a time) through the DEFAULT flow
        try:
            extra['per_image_B100_reference_flow'] = per_image_latency(torch, syn, dev, batch0, args, reference_flow=True)
        except Exception as e:                                          # noqa: BLE001 — secondary figure
            extra['per_image_B100_reference_flow'] = {'error': repr(e)}
    # reference flow: how one call splits into the initialiser's launches and the LM launch (HIP events on the launch stream, every batch)
    split = None
    if ref_flow and args.full:
        lib_ = launches_one[0][0].lib
        st_ = torch.cuda.current_stream(dev).cuda_stream
        ev3 = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(2 * NB)]
        torch.cuda.synchronize()
        for i, (a, b, c) in enumerate(ev3):
            l = launches_one[i % NB][0]
            g1 = l._single                          # the launch set of one call the launch object runs (re-fit deferred into the LM launch)
            a.record(); lib_.mr_epnp_ransac_grouped(*g1.args, st_); b.record(); lib_.mr_pnp_uncert_from_epnp_grouped(*g1.args_fused, st_); c.record()
        torch.cuda.synchronize()
        ini_ms = np.array([a.elapsed_time(b) for a, b, c in ev3[NB:]]); lm_ms = np.array([b.elapsed_time(c) for a, b, c in ev3[NB:]])
        split = {'initialiser_launches_ms': float(ini_ms.mean()), 'lm_launch_ms': float(lm_ms.mean()), 'lm_launch_ms_per_batch': [float(v) for v in lm_ms],
                 'what': 'one call at a time, HIP events on the launch stream around the launches of mr_epnp_ransac_grouped (MR_EPNP_DEFER_REFIT: front, hypotheses, consensus, second round, re-fit betas — five for a call of fewer than 2048 objects, six for a launch set) and around the LM launch that carries the re-fit (mr_pnp_uncert_from_epnp_grouped), averaged over the batches'}

    if rank == 0:
        total = B_PER_GPU * world * args.steps
        ms_per_step = elapsed / args.steps * 1e3
        line = {
            'metric': 'PnP solves/sec (1024 proposals, 28x28 corr.)' if not stress else 'PnP solves/sec (stress: 8192 proposals/GPU, 56x56 corr., fp16 storage)', 'value': total / elapsed, 'unit': 'solves/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': ms_per_step,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
            'config': {'workload': ('BASELINE config 2: 1024 synthetic proposals x 28x28 2D-3D correspondences with per-point '
                                    'istd, fp32 storage, channel-planar (NCHW-view) layout, per GPU') if not stress else
                                   ('BASELINE config 5 shard: 8192 synthetic proposals x 56x56 correspondences, fp16 storage, '
                                    'channel-planar layout, per GPU (1024 distinct objects tiled 8x)'),
                       'objects_per_gpu': B_PER_GPU, 'points_per_object': P, 'seed': SEED,
                       'resident_batches': NB, 'resident_input_bytes': resident_bytes,
                       'batch_rotation': f'steps rotate over {NB} distinct batches (seeds {seeds[0]}, {seeds[0]}+7919*i); {resident_bytes / 2**20:.0f} MiB of inputs '
                                         'resident, more than the 256 MiB Infinity Cache' + (f'; every rank holds the same {NB} batches and starts '
                                         f'the rotation at offset rank*{NB}//{world} (distinct batches across ranks at every step, equal work per rotation)' if world > 1 else ''),
                       'flow': ("reference: the drop-in boundary's default — PnPUncert built from the reference's config dict (configs/kitti_car.py:118-126)" if ref_flow else
                                "k0: the explicit fast mode, PnPUncert(initialiser='k0')"),
                       'stages': ('istd mask + cv2.solvePnPRansac(EPNP, 30 iterations) restated (front / hypotheses / consensus / re-fit launches) + LM (Ceres-1.14 semantics, fp64) '
                                  '+ covariance: ' + LAUNCHES_TEXT + ' (the last one = the re-fit\'s pose candidates, then LM + covariance)' if ref_flow else
                                  'istd mask + K0 consensus initialiser (32 hyp.) + LM (Ceres-1.14 semantics, fp64) + covariance: one fused launch'),
                       'calls_per_launch_set': LG,
                       'launches_in_flight': L, 'launches_in_flight_asked': L_ASKED, 'stream_overlap_test': pipe_of(L_ASKED).overlap_test, 'waves_per_object': {'in_flight': (fl_main >> 8) & 15 or 'library heuristic (4)', 'isolated_launch': (fl_one >> 8) & 15 or 'library heuristic (4)'},
                       'issue': ((f'steps issued on {L} HIP streams by monorun_amd.PnPPipeline, {LG} consecutive steps per launch set (monorun_amd.PnPEpnpGroupLaunch: the '
                                  "every launch of the set — the initialiser's six and the re-fit / LM / covariance launch: seven — carries the objects of the set's calls, every call keeps its own input tensors and result buffers); "
                                  if LG > 1 else f'steps issued round-robin on {L} HIP streams by monorun_amd.PnPPipeline (one completion event per result buffer); ') +
                                 f'every step is one full {B_PER_GPU}-object call into its own buffers, all outputs complete inside the timed window' +
                                 (' and verified bit-identical to isolated calls after it' if args.full else '')) if L > 1 else 'one stream: every launch waits for the previous one',
                       'prewarm': dict(prewarm, what='untimed launches of the same hot path before the W warm-up steps, so that the timed window does not start on idle clocks (MR_BENCH_PREWARM_LAUNCHES=0 disables)'),
                       'parallelism': f'objects sharded x{world}' + (f', 1 all-gather of 88 B/object x {comm["steps_per_collective"]} step(s) per collective' if (world > 1 and comm) else '')},
            'value_cold': prewarm.get('window_before', {}).get('value'),      # the same window in a just-started process (before the reported pre-conditioning): compare THIS with rounds 1-3
            'valid_fraction': valid_frac,
        }
        if args.full:
            achieved = BYTES_PER_SOLVE * B_PER_GPU / (kernel_ms * 1e-3) / 1e9
            traffic, traffic_src, traffic_iso = None, None, None
            tfile = os.path.join(ROOT, 'profiles', 'traffic.json')   # HBM bytes per launch from the PMC passes (see profiles/README.md)
            def newest(pattern):                     # the newest committed profile of this name (profiles/rNN_<pattern>), or None
                import glob
                c = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_' + pattern)), reverse=True)
                return c[0] if c else None
            if ref_flow:
                tf = newest('epnp_traffic_stress.json' if stress else 'epnp_traffic.json')
                if tf:
                    try:
                        tj = json.load(open(tf))
                        traffic = traffic_iso = tj.get('hbm_bytes_per_call')
                        traffic_src = (f'profiles/{os.path.basename(tf)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over all launches of one call, one call at a time, committed; '
                                       f'{tj.get("ratio_traffic_over_algorithmic", 0):.2f} x the algorithmic bytes); replayed, not measured in this run')
                    except Exception:  # noqa: BLE001
                        traffic = traffic_iso = None
            elif os.path.exists(tfile) and not stress:
                try:
                    tj = json.load(open(tfile))
                    traffic_iso = tj.get('hbm_bytes_per_launch')
                    traffic_fl = (tj.get('in_flight_kernel') or {}).get('hbm_bytes_per_launch')
                    traffic = traffic_fl if (L > 1 and traffic_fl) else traffic_iso
                    traffic_src = ('profiles/traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, tools/profile_round.sh ' + str(tj.get('tag', '')) + ', committed: ' +
                                   ('the 2-waves-per-object kernel the timed region launches, counted on isolated launches of it' if (L > 1 and traffic_fl) else 'the isolated-launch kernel') +
                                   '); replayed, not measured in this run')
                except Exception:  # noqa: BLE001
                    traffic = None
            valu = None
            if ref_flow and not stress:
                vf = newest('epnp_valu_per_launch.json')
                if vf:
                    try:
                        vj = json.load(open(vf))
                        cnt = float(vj['valu_insts_per_call'])
                        t_min = cnt * 4.0 / (1024 * 2.4e9)
                        valu = {'valu_insts_per_call': cnt, 'min_issue_time_us_at_4_cycles': t_min * 1e6, 'frac_of_call_time': t_min / (kernel_ms * 1e-3),
                                'per_launch': vj.get('per_launch'),
                                'source': f'profiles/{os.path.basename(vf)} (rocprofv3 --pmc SQ_INSTS_VALU over the launches of one call, one call at a time, committed); replayed, not measured in this run'}
                    except Exception:  # noqa: BLE001
                        valu = None
            for sname in ('r04_summary.json', 'r03_summary.json', 'r02_summary.json', 'r01_summary.json'):           # PMC instruction counts of the same command
                sfile = os.path.join(ROOT, 'profiles', sname)
                if os.path.exists(sfile) and not stress and not ref_flow:
                    try:
                        sj = json.load(open(sfile))
                        cnt = (sj['single_stream'] if 'single_stream' in sj else sj)['counters']['SQ_INSTS_VALU']['mean']      # the isolated (4-wave) kernel
                        # every VALU wave-instruction occupies its SIMD for >= 2 (fp32) .. 4 (fp64) cycles; 1024 SIMDs at 2.4 GHz
                        t_min = cnt * 4.0 / (1024 * 2.4e9)
                        valu = {'valu_insts_per_launch': cnt, 'min_issue_time_us_at_4_cycles': t_min * 1e6,
                                'frac_of_kernel_time': t_min / (kernel_ms * 1e-3),
                                'source': f'profiles/{sname} (rocprofv3 --pmc SQ_INSTS_VALU, committed); replayed, not measured in this run'}
                        break
                    except Exception:  # noqa: BLE001
                        valu = None
            flops_ach = flops_per_launch / (kernel_ms * 1e-3) / 1e12
            line['roofline'] = {'bound': 'hbm', 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                                # filled in below: `achieved` / `frac` describe the TIMED REGIME (the kernel instantiation and issue pattern `value` was measured on)
                                'achieved': None, 'frac': None,
                                'kernel': (f'reference flow, ' + LAUNCHES_TEXT + f' (epnp_front / epnp_hyp / epnp_consensus / second round: epnp_round2 or epnp_hyp + epnp_consensus / epnp_refit_betas / pnp_uncert_refit_kernel<{"__half" if stress else "float"}, {((fl_main >> 8) & 15) or 4}>); longest: the last one (re-fit prologue + LM + covariance)' if ref_flow else
                                           (f'pnp_uncert_kernel<float, {((fl_main >> 8) & 15) or 4}, false>' if not stress else f'pnp_uncert_kernel<__half, {((fl_main >> 8) & 15) or "auto"}, false>')),
                                'launches_in_flight': L,
                                'traffic': traffic, 'traffic_source': traffic_src,
                                'algorithmic_bytes_per_launch': BYTES_PER_SOLVE * B_PER_GPU,
                                'isolated_launch': {
                                    'achieved': achieved, 'frac': achieved / HBM_PEAK_GBS, 'unit': 'GB/s',
                                    'kernel': ('one whole call of the reference flow (its 6 launches back to back on one stream)' if ref_flow else
                                               (f'pnp_uncert_kernel<float, {((fl_one >> 8) & 15) or 4}, false>' if not stress else 'pnp_uncert_kernel<__half, auto, false>')),
                                    'kernel_ms_avg': kernel_ms, 'kernel_ms_min': float(k_ms.min()),
                                    'kernel_ms_median': float(np.median(k_ms)), 'kernel_ms_p95': float(np.percentile(k_ms, 95)), 'kernel_ms_per_batch': per_batch_ms,
                                    'measured_on': 'HIP events around ISOLATED launches on one stream (the library\'s own choice there: 4 waves per object), rotating over the '
                                                   'batches, in this run; rocprofv3 of `bench.py --in-flight 1` agrees (profiles/rNN_kernel_stats.csv).  NOT the instantiation the '
                                                   'timed region launches when launches_in_flight > 1',
                                    'batch0_only': {'kernel_ms': per_batch_ms[0], 'frac': BYTES_PER_SOLVE * B_PER_GPU / (per_batch_ms[0] * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                                    'note': 'batch 0 (the config seed) alone; a launch lasts as long as its slowest object, so batches differ'},
                                    'traffic': traffic_iso, 'valu_issue': valu},
                                'flops': {'fp64_flop_per_launch': flops_per_launch, 'achieved_tflops': flops_ach, 'peak_tflops': FP64_VECTOR_PEAK_TFLOPS,
                                          'frac_of_fp64_vector_peak': flops_ach / FP64_VECTOR_PEAK_TFLOPS,
                                          'model': f'{FLOP_PER_POINT_EVAL} FLOP x inlier points x (LM iterations + 2) per object (SURVEY 8d; iterations and inlier '
                                                   'counts read back from the kernel in this run); K0 and the mask are not counted; rate per ISOLATED launch',
                                          'lm_iteration_histogram': {str(k): it_hist[k] for k in sorted(it_hist)}},
                                'note': ('formally HBM-bound (three of the launches stream the object\'s rows once each); in practice the stages are serial fp64 latency chains per object one call at a time, '
                                         'and issue slots x workgroup residency with launch sets in flight (wave-instruction counts per launch: `isolated_launch.valu_issue`, DESIGN.md section 3)' if ref_flow else
                                         'formally HBM-bound (read-once streaming); in practice VALU/latency-bound: the tile is LDS-resident across all LM iterations (DESIGN.md)')}
            line['outputs_verified'] = outputs_ok
            line['secondary_throughput'] = extra
            def per_s(v):
                return {'value': B_PER_GPU * world * v['steps'] / v['elapsed'], 'unit': 'solves/s', 'ms_per_step': v['elapsed'] / v['steps'] * 1e3, 'steps': v['steps']}
            rn = per_s(variants['rotation_normalised'])
            line['value_rotation_normalised'] = rn['value']
            line['rotation_normalised'] = dict(rn, what=f'the same loop timed over {rn["steps"]} steps = a whole number of rotations over the {NB} batches '
                                                        '(--steps need not be a multiple of --batches, and the batches take different times)')
            if 'single_stream' in variants:
                line['single_stream'] = dict(per_s(variants['single_stream']), what=('ONE CALL AT A TIME: the same steps on one stream, every call (its 6 launches) waits for the previous one'
                                             if ref_flow else 'the same steps on ONE stream (launches_in_flight = 1): every launch '
                                             'waits for the previous one and so pays its slowest object; what rounds 1-2 reported as `value`'))
            if 'grouped_collective' in variants:
                extra['grouped_collective'] = dict(per_s(variants['grouped_collective']), steps_per_collective=variants['grouped_collective']['steps_per_collective'],
                                                   what='the same loop with the other exchange granularity (one all-gather per this many steps)')
            chip = line['value'] / world * BYTES_PER_SOLVE / 1e9          # per GPU: algorithmic bytes of all launches / wall time of the timed region
            line['roofline']['achieved'], line['roofline']['frac'] = chip, chip / HBM_PEAK_GBS
            line['roofline']['measured_on'] = (
                f'the timed region itself: algorithmic bytes of its {args.steps} launches / its wall time, per GPU ({L} launches in flight on '
                f'{L} HIP streams, {((fl_main >> 8) & 15) or 4} waves per object) — launches overlap, so the chip-level rate is what a roofline fraction '
                'can mean here; per-launch figures of an isolated launch are under `isolated_launch`') if L > 1 else \
                'one launch at a time: algorithmic bytes / wall time of the timed region (per-launch HIP-event figures under `isolated_launch`)'
            if k_fl_ms is not None:
                line['roofline']['launch_resident_ms_in_flight'] = {
                    'avg': float(k_fl_ms.mean()), 'median': float(np.median(k_fl_ms)), 'min': float(k_fl_ms.min()), 'launches': int(len(k_fl_ms)),
                    'what': 'HIP events on the pipeline\'s own streams around every launch of a 240-step run of the timed issue pattern: how long a launch is '
                            f'resident while {L} overlap (avg / {L} = chip time per launch); agrees with profiles/rNN_kernel_stats_in_flight.csv'}
            ss = per_s(variants['steady_state'])
            line['steady_state'] = dict(ss, frac=ss['value'] / world * BYTES_PER_SOLVE / 1e9 / HBM_PEAK_GBS,
                                        what=f'the timed loop over {ss["steps"]} steps (whole rotations): the {args.steps}-step window of `value` carries the fill and drain of the {L}-deep pipeline')
            if ref_flow:
                one = per_s(variants['single_stream']) if 'single_stream' in variants else None
                lm_name = f'pnp_uncert_refit_kernel<{"__half" if stress else "float"}, {((fl_one >> 8) & 15) or ("auto" if stress else 4)}>'
                line['reference_flow'] = {
                    'what': "`value` IS this flow since round 5: cv2.solvePnPRansac(EPNP, 30 iterations) restated on the GPU, then the LM + covariance — what PnPUncert built from the "
                            "reference's own config dict runs (INTEGRATION.md section 2); the one-launch K0 path is the explicit fast mode (`k0_fast_mode`)",
                    'in_flight': {'value': line['value'], 'unit': 'solves/s', 'launches_in_flight': L, 'calls_per_launch_set': LG, 'steady_state': ss['value']},
                    'one_call_at_a_time': one, 'launch_split': split,
                    'per_image_B100': extra.pop('per_image_B100_reference_flow', None)}
                if split is not None:
                    # the longest launch of the call: the LM launch (its length is its slowest object's: up to 35 LM iterations from EPnP starts)
                    ach = BYTES_PER_SOLVE * B_PER_GPU / (split['lm_launch_ms'] * 1e-3) / 1e9
                    line['roofline']['dominant_kernel'] = {'kernel': lm_name, 'avg_launch_ms': split['lm_launch_ms'], 'achieved': ach, 'unit': 'GB/s', 'frac': ach / HBM_PEAK_GBS,
                                                           'algorithmic_bytes_per_launch': BYTES_PER_SOLVE * B_PER_GPU,
                                                           'measured_on': "HIP events on the launch stream around ISOLATED launches of the LM kernel (one call at a time; the launch also carries the initialiser's re-fit as its prologue), every batch, in this run"}
            if isinstance(extra.get('epnp_initialiser'), dict) and 'value' in extra['epnp_initialiser']:
                ep = extra['epnp_initialiser']
                line['reference_flow'] = {
                    'what': "the reference's own flow on the GPU — cv2.solvePnPRansac(EPNP, 30 iterations) restated, then the LM + covariance: PnPUncert(initialiser='epnp'); "
                            "`value` above is the one-launch K0 path, which is NOT the reference's initialiser (INTEGRATION.md section 2)",
                    'value': ep['value'], 'unit': 'solves/s', 'ms_per_step': ep['ms_per_step'], 'issue': ep.get('issue'),
                    'synchronous_call': ep.get('synchronous_call'), 'in_flight': ep.get('in_flight'), 'roofline': ep.get('roofline'),
                    'launch_split_batch0_ms': {'initialiser': ep.get('epnp_ransac_launches_ms_batch0'), 'lm': ep.get('lm_launch_ms_batch0')}}
            line['roofline']['in_flight'] = {
                'launches_in_flight': L, 'achieved': line['value'] / world * BYTES_PER_SOLVE / 1e9, 'unit': 'GB/s',
                'frac': line['value'] / world * BYTES_PER_SOLVE / 1e9 / HBM_PEAK_GBS,
                'note': 'chip-level rate of the timed region: algorithmic bytes of ALL launches / wall time (launches overlap, so this is not a '
                        'per-launch duration); `achieved` / `frac` above are per launch, from HIP events around isolated launches on one stream'}
        if comm is not None:
            if args.full:
                comm['gathered_rows_verified'] = gather_ok
            line['comm'] = comm
        if dumped is not None:
            line['outputs_dumped'] = dumped
        if args.full and ref_flow and world == 1 and not args.no_secondary and not stress:
            # the explicit fast mode, measured by the same script in a child process (the parent is idle meanwhile): rounds 1-4's `value`
            import subprocess
            import tempfile
            fd, kfile = tempfile.mkstemp(prefix='mr_bench_k0_', suffix='.json')
            os.close(fd)
            cmd = [sys.executable, os.path.abspath(__file__), '--flow', 'k0', '--steps', str(args.steps), '--warmup', str(args.warmup), '--batches', str(args.batches),
                   '--in-flight', str(args.in_flight), '--full', '--no-cpu-baseline', '--details', kfile]
            try:
                torch.cuda.synchronize()
                cp = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, MR_BENCH_SKIP_EPNP_SECONDARY='1'))
                with open(kfile) as f:
                    kj = json.loads(f.read())
                line['k0_fast_mode'] = {
                    'what': "PnPUncert(initialiser='k0'): this repository's one-launch consensus initialiser fused with the LM — NOT the reference's initialiser "
                            '(inlier sets differ from the reference flow\'s on ~13 % of config-2 objects); `python bench.py --full --flow k0 --details FILE` writes this record on its own',
                    'value': kj['value'], 'unit': 'solves/s', 'ms_per_step': kj['ms_per_step'], 'steps': kj['steps'], 'steady_state': kj.get('steady_state'),
                    'single_stream': kj.get('single_stream'), 'roofline': kj.get('roofline'), 'config': {k: kj['config'].get(k) for k in ('stages', 'launches_in_flight', 'waves_per_object', 'prewarm')},
                    'secondary_throughput': kj.get('secondary_throughput')}
            except Exception as e:  # noqa: BLE001
                line['k0_fast_mode'] = {'error': repr(e)}
            finally:
                os.remove(kfile)
        if args.full and world == 1 and not args.no_cpu_baseline:
            cb = cpu_baseline(np_batch0, perturbed_gt_init(batch0, SEED) if not stress else None, args.cpu_seconds, ref_flow,
                              'config-2 batch 0' if not stress else 'the stress batch (56x56 correspondences; float32 values, the GPU reads them rounded to fp16)')
            line.update(cb)
            if ref_flow and isinstance(line.get('k0_fast_mode'), dict) and 'value' in line['k0_fast_mode'] and 'cpu_baseline_k0' in cb:
                line['k0_fast_mode']['speedup_vs_cpu_k0_1thread'] = line['k0_fast_mode']['value'] / cb['cpu_baseline_k0']['value']
            line['speedup_vs_cpu_1thread'] = line['value'] / cb['cpu_baseline']['value']
            line['speedup_vs_cpu_all_cores'] = line['value'] / cb['cpu_baseline_all_cores']['value']
            if 'cpu_baseline_epnp' in cb:
                line['speedup_vs_cpu_epnp_1thread'] = line['value'] / cb['cpu_baseline_epnp']['value']
            if 'cpu_baseline_epnp' in cb and 'reference_flow' in line and 'value' in line['reference_flow']:
                line['reference_flow']['cpu_baseline_epnp'] = cb['cpu_baseline_epnp']
                line['reference_flow']['speedup_vs_cpu_epnp_1thread'] = line['reference_flow']['value'] / cb['cpu_baseline_epnp']['value']
            if ref_flow and line['reference_flow'].get('one_call_at_a_time'):
                line['reference_flow']['one_call_at_a_time']['speedup_vs_cpu_1thread'] = line['reference_flow']['one_call_at_a_time']['value'] / cb['cpu_baseline']['value']
            if 'cpu_baseline_epnp' in cb and 'value' in extra.get('epnp_initialiser', {}):
                line['speedup_epnp_initialiser_vs_cpu_epnp_1thread'] = extra['epnp_initialiser']['value'] / cb['cpu_baseline_epnp']['value']
            if 'init_given' in extra:
                line['speedup_init_given_vs_cpu_1thread'] = extra['init_given']['value'] / cb['cpu_baseline_init_given']['value']
        if args.details:
            with open(args.details, 'w') as f:
                f.write(json.dumps(line) + '\n')
        _emit(headline(line))
    if rccl is not None:
        rccl.close()
    if use_dist:
        dist.destroy_process_group()


def secondary(args, torch, syn, PnPLaunch, dev, dev_batches, batch0, np_batch0, NB):
    """Secondary, clearly labelled figures (never `value`)."""
    extra = {}
    fl = args.waves << 8
    x2d, istd, x3d, K, ur, vr, thr = dev_batches[0]

    def mk(b, **kw):
        return PnPLaunch(b[0], b[1], b[2], b[3], b[4], b[5], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=b[6], inlier_opt_only=True, flags=fl, **kw)
    # (a) the same steps issued round-robin on 4 HIP streams (independent batches in flight, as a serving loop would): at
    #     B = 1024 a launch lasts as long as its slowest object, streams fill the idle SIMDs of the tail
    n_str = 4
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_str)]
    ls = [mk(dev_batches[i % NB]) for i in range(max(n_str, NB))]
    for i in range(2 * n_str):
        ls[i % len(ls)].run(streams[i % n_str].cuda_stream)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i in range(args.steps):
        ls[i % len(ls)].run(streams[i % n_str].cuda_stream)
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    extra['pipelined_4_streams'] = {'value': B_PER_GPU * args.steps / el, 'unit': 'solves/s', 'ms_per_step': el / args.steps * 1e3}
    # (b) one launch over 8 batches (8192 objects): the kernel's throughput regime
    nb8 = min(8, NB)
    cat = lambda j, c: torch.cat([dev_batches[i % NB][j].permute(0, 2, 1).contiguous() for i in range(8)], 0).permute(0, 2, 1)   # planar views kept
    big = (cat(0, 2), cat(1, 2), cat(2, 3), K, ur, vr, torch.cat([dev_batches[i % NB][6] for i in range(8)]))
    lb = mk(big)
    for _ in range(3):
        lb.run()
    torch.cuda.synchronize()
    nb = max(4, args.steps // 8)
    t1 = time.perf_counter()
    for _ in range(nb):
        lb.run()
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    extra['single_launch_8192_objects'] = {'value': 8 * B_PER_GPU * nb / el, 'unit': 'solves/s', 'ms_per_launch': el / nb * 1e3, 'distinct_batches': nb8}
    del lb, big
    # (c) initialiser excluded: init_pose given (GT + seeded perturbation), istd mask + LM + covariance only
    ini = torch.from_numpy(perturbed_gt_init(batch0, SEED)).to(dev)
    li = mk(dev_batches[0], init_pose=ini)
    for _ in range(5):
        li.run()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(args.steps):
        li.run()
    torch.cuda.synchronize()
    el = time.perf_counter() - t1
    extra['init_given'] = {'value': B_PER_GPU * args.steps / el, 'unit': 'solves/s', 'ms_per_step': el / args.steps * 1e3,
                           'what': 'K0 excluded: init_pose = GT + seeded perturbation (sigma 0.1 rad / 0.3 / 0.1 / 1.0 m), batch 0; the CPU '
                                   'counterpart is cpu_baseline_init_given'}
    # (e) the optional second launches on batch 0: 6-DoF refinement (use_6dof=True) and the exact Hessian (forward_exact_hessian=True)
    try:
        from monorun_amd.ops.least_squares.pnp_uncert import pnp6_refine_device, exact_hessian_device
        l0 = mk(dev_batches[0])
        l0.run()
        torch.cuda.synchronize()
        mask_u8, pose4, valid4 = l0.mask.clone(), l0.pose.clone(), l0.valid.clone()

        def timed(fn, n):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t1) / n
        n2 = max(10, args.steps // 4)
        t6 = timed(lambda: pnp6_refine_device(x2d, istd, x3d, K, ur, vr, mask_u8, pose4, valid4, z_min=0.5), n2)
        th = timed(lambda: exact_hessian_device(x2d, istd, x3d, K, ur, vr, pose4, mask_u8, valid4, z_min=0.5), n2)
        extra['second_launches'] = {
            'six_dof_refine': {'ms_per_call': t6 * 1e3, 'value': B_PER_GPU / t6, 'unit': 'refinements/s'},
            'exact_hessian': {'ms_per_call': th * 1e3, 'value': B_PER_GPU / th, 'unit': 'objects/s'},
            'what': 'host wall per call incl. output allocation and argument marshalling, 1024 objects, after the 4-DoF solve of batch 0'}
    except Exception as e:                                          # noqa: BLE001 — secondary figure
        extra['second_launches'] = {'error': repr(e)}
    # (g) the reference's own flow on the GPU (PnPUncert(initialiser='epnp')): EPnP / RANSAC initialiser launches + LM launch, next to
    #     cpu_baseline_epnp.  `value`: prepared launches (PnPEpnpLaunch: outputs, hand-over buffers and workspace allocated once) issued
    #     back to back on ONE stream, rotating over the batches — at most one call executes at any time, the host only enqueues;
    #     `synchronous_call`: the eager op with a host synchronisation after every call (what round 3 reported as `value`);
    #     `in_flight`: the same prepared launches on PnPPipeline's streams.
    try:
        if os.environ.get('MR_BENCH_SKIP_EPNP_SECONDARY') == '1':      # the parent run measures that flow as its `value`
            raise StopIteration
        from monorun_amd.ops.least_squares.pnp_uncert import epnp_ransac_device, pnp_uncert_from_init_device
        from monorun_amd import PnPEpnpLaunch, PnPPipeline
        mk_ep = lambda bi, fl=0: PnPEpnpLaunch(*dev_batches[bi % NB][:6], z_min=0.5, epnp_istd_thres=0.6, epnp_ransac_thres=dev_batches[bi % NB][6],
                                               inlier_opt_only=True, flags=fl)
        nrot = NB                     # every resident batch: ~15 % of config-2 batches hold an object whose RANSAC loop wants more than the 8 first-round hypotheses
        le1 = [mk_ep(i) for i in range(nrot)]
        for l in le1:
            l.run()
        torch.cuda.synchronize()
        ne = max(24, args.steps)
        ne -= ne % nrot
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        t1 = time.perf_counter()
        for i in range(ne):
            le1[i % nrot].run()
        torch.cuda.synchronize()
        el = time.perf_counter() - t1
        # the split of one call: HIP events on the launch stream around the initialiser's launches and the LM launch, batch 0
        t_init = t_lm = 0.0
        for _ in range(6):
            evs[0].record(); le1[0].lib.mr_epnp_ransac_batched(*le1[0].args_init, torch.cuda.current_stream().cuda_stream)
            evs[1].record(); le1[0].lib.mr_pnp_uncert_from_init_batched(*le1[0].args_lm, torch.cuda.current_stream().cuda_stream)
            evs[2].record(); torch.cuda.synchronize()
            t_init += evs[0].elapsed_time(evs[1]) / 6; t_lm += evs[1].elapsed_time(evs[2]) / 6
        ref = pnp_uncert_from_init_device(*dev_batches[0][:6], *epnp_ransac_device(*dev_batches[0][:4], epnp_istd_thres=0.6, epnp_ransac_thres=dev_batches[0][6])[:3],
                                          z_min=0.5, inlier_opt_only=True)
        torch.cuda.synchronize()
        same1 = bool(torch.equal(le1[0].pose, ref[1]) and torch.equal(le1[0].mask, ref[4]) and torch.equal(le1[0].valid, ref[0]))
        ep = {'value': B_PER_GPU * ne / el, 'unit': 'solves/s', 'ms_per_step': el / ne * 1e3, 'steps': ne, 'distinct_batches': nrot,
              'epnp_ransac_launches_ms_batch0': t_init, 'lm_launch_ms_batch0': t_lm, 'valid': int(ref[0].sum().item()),
              'outputs_equal_the_eager_op': same1,
              'issue': 'prepared launches (PnPEpnpLaunch) back to back on ONE stream, no host synchronisation between calls: one call at a time on the device',
              'what': "pnp_uncert(..., initialiser='epnp'): the reference's initialiser (30 EPnP hypotheses on cv::RNG subsets, consensus, adaptive "
                      'iteration count, EPnP re-fit) as seven launches, then the LM + covariance launch; masks and poses equal the CPU '
                      'restatement (tests/test_gpu_epnp.py); the CPU counterpart is cpu_baseline_epnp'}
        # the eager op, one host synchronisation per call (allocations + argument marshalling + the synchronisation inside the figure)
        ns = max(8, args.steps // 2)
        t1 = time.perf_counter()
        for _ in range(ns):
            ini, im, iv, _, _ = epnp_ransac_device(x2d, istd, x3d, K, epnp_istd_thres=0.6, epnp_ransac_thres=thr)
            out = pnp_uncert_from_init_device(x2d, istd, x3d, K, ur, vr, ini, im, iv, z_min=0.5, inlier_opt_only=True)
            torch.cuda.synchronize()
        el = time.perf_counter() - t1
        ep['synchronous_call'] = {'value': B_PER_GPU * ns / el, 'unit': 'solves/s', 'ms_per_step': el / ns * 1e3, 'steps': ns,
                                  'what': 'the eager op on batch 0 with torch.cuda.synchronize() after every call (round 3 reported this as `value`)'}
        extra['epnp_initialiser'] = ep
        # the same flow with prepared launches in flight (PnPPipeline): the stages are latency chains, several batches overlap
        pipe = PnPPipeline(dev, depth=4, record_events=False)
        nl = max(pipe.depth, 1)
        nobj = ((max(NB, nl) + nl - 1) // nl) * nl                              # launch objects: a multiple of the depth, so that object i always lands on stream i % depth
        le = [mk_ep(i, pipe.flags_for(B_PER_GPU, P)) for i in range(nobj)]     # the LM launch with the waves per object the pipeline asks for
        for i in range(nobj):
            pipe.submit(le[i], slot=i % nl)
        pipe.drain()
        nf = max(96, 4 * args.steps)
        nf -= nf % nobj
        t1 = time.perf_counter()
        for i in range(nf):
            pipe.submit(le[i % nobj], slot=(i % nobj) % nl)
        pipe.drain()
        el = time.perf_counter() - t1
        same = bool(torch.equal(le[0].pose, ref[1]) and torch.equal(le[0].mask, ref[4]) and torch.equal(le[0].valid, ref[0]))
        ep['in_flight'] = {'value': B_PER_GPU * nf / el, 'unit': 'solves/s', 'ms_per_step': el / nf * 1e3, 'launches_in_flight': nl, 'steps': nf,
                           'distinct_batches': min(nobj, NB), 'outputs_equal_the_one_at_a_time_results': same,
                           'what': 'PnPEpnpLaunch objects (initialiser + LM, own workspace and outputs) submitted round-robin to PnPPipeline'}
        # roofline of the flow: the algorithmic bytes are config 2's (every correspondence read once, the outputs written once); the
        # launches re-read the tile (front, consensus, re-fit, LM: 4 x) and hand over through a 17 MB workspace — HBM traffic from the
        # PMC passes is replayed from profiles/ when present
        alg = BYTES_PER_SOLVE * B_PER_GPU
        rf = {'bound': 'hbm', 'unit': 'GB/s', 'peak': HBM_PEAK_GBS, 'algorithmic_bytes_per_call': alg,
              'achieved': alg / (ep['ms_per_step'] * 1e-3) / 1e9, 'frac': alg / (ep['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS,
              'in_flight': {'achieved': alg / (ep['in_flight']['ms_per_step'] * 1e-3) / 1e9, 'frac': alg / (ep['in_flight']['ms_per_step'] * 1e-3) / 1e9 / HBM_PEAK_GBS},
              'traffic': None,
              'note': 'latency-bound: each of the eight launches is a serial chain per object (Jacobi SVDs, Gauss-Newton, bisection) that leaves most issue slots idle; '
                      'the per-launch table is profiles/r04_epnp_launches.txt'}
        tfile = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'r04_epnp_traffic.json')
        if os.path.exists(tfile):
            try:
                tj = json.load(open(tfile))
                rf['traffic'] = tj.get('hbm_bytes_per_call')
                rf['traffic_source'] = 'profiles/r04_epnp_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/gpu_epnp_path.py, committed); replayed, not measured in this run'
            except Exception:  # noqa: BLE001
                pass
        ep['roofline'] = rf
        del le, le1
    except StopIteration:
        pass
    except Exception as e:                                          # noqa: BLE001 — secondary figure
        extra['epnp_initialiser'] = {'error': repr(e)}
    # (f) the NOC path at B = 1024: raw head output -> pose, fused (one launch) and as two launches (K2 decode, then the PnP kernel)
    try:
        extra['head_to_pose_1024'] = head_to_pose(torch, syn, PnPLaunch, dev)
    except Exception as e:                                          # noqa: BLE001 — secondary figure
        extra['head_to_pose_1024'] = {'error': repr(e)}
    # (d) the deployment regime (monorun_roi_head.py:452: one image per forward, <= 100 proposals): per-call latency
    try:
        extra['per_image_B100'] = per_image_latency(torch, syn, dev, batch0, args)
    except Exception as e:                                          # noqa: BLE001 — secondary figure: report, do not fail the line
        extra['per_image_B100'] = {'error': repr(e)}
    return extra


def graph_us_per_launch(torch, fns, reps=20):
    """Average GPU time of one launch of `fns` (a list of enqueue-only callables) when they run back to back: the sequence is
    captured into ONE HIP graph and replayed `reps` times between two events — no host launch latency between the kernels, the
    ~1.5 us kernel boundary included."""
    for f in fns:
        f()                                                          # warm-up outside the capture (LDS opt-in, lazy module load)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(fns))


def roof_of(nbytes, us):
    ach = nbytes / (us * 1e-6) / 1e9
    return {'bound': 'hbm', 'achieved': ach, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': ach / HBM_PEAK_GBS, 'algorithmic_bytes_per_launch': nbytes}


def head_to_pose_reference(torch, syn, dev, n_batches=4):
    """The whole post-NOC-head tail as the pipeline's head built from the REFERENCE's config dict runs it (monorun_roi_head.py:509-534): K2
    decode -> the reference's initialiser -> LM -> calibration, prepared launches (PoseFromHeadLaunch) over 4 distinct resident head
    outputs, one at a time and four in flight."""
    from monorun_amd.pose_head import PoseFromHeadLaunch, UncertPropPnPOptimizer
    from monorun_amd import PnPPipeline
    head = UncertPropPnPOptimizer().to(dev)
    ls = []
    for i in range(n_batches):
        b = syn.make_batch(B=B_PER_GPU, hw=HW, seed=SEED + 7919 * i)
        all_pred, dim = syn.encode_head_outputs(b, seed=SEED + i)
        ls.append(PoseFromHeadLaunch(head, torch.from_numpy(all_pred).to(dev), torch.from_numpy(b['labels']).to(dev), False, torch.from_numpy(dim).to(dev), None,
                                     torch.from_numpy(b['rois']).to(dev), torch.from_numpy(b['K']).to(dev), (syn.IMG_H, syn.IMG_W)))
    out = {'what': "PoseFromHeadLaunch of a head built from the reference's config dict: K2 decode + EPnP / RANSAC initialiser + LM + calibration, 1024 objects per call"}
    for name, depth in (('one_call_at_a_time', 1), ('in_flight', 4)):
        pipe = PnPPipeline(dev, depth=depth, record_events=False)
        for i in range(2 * n_batches):
            pipe.submit(ls[i % n_batches], slot=i % n_batches)
        pipe.drain()
        n = 48
        t0 = time.perf_counter()
        for i in range(n):
            pipe.submit(ls[i % n_batches], slot=i % n_batches)
        pipe.drain()
        el = time.perf_counter() - t0
        out[name] = {'value': B_PER_GPU * n / el, 'unit': 'solves/s', 'us_per_call': el / n * 1e6, 'launches_in_flight': pipe.depth}
    out['valid_fraction'] = float(ls[0].out['ret_val'].float().mean().item())
    # launch sets (PoseFromHeadGroupLaunch): four sets of four calls on four streams — sixteen launch objects with their own decoded maps
    # and outputs over the four resident head outputs
    from monorun_amd.pose_head import PoseFromHeadGroupLaunch
    inp = [l.inputs for l in ls]
    more = [PoseFromHeadLaunch(head, inp[i % n_batches]['all_pred'], inp[i % n_batches]['labels'], False, inp[i % n_batches]['dim'], None, inp[i % n_batches]['rois'],
                               inp[i % n_batches]['cam_intrinsic'], (syn.IMG_H, syn.IMG_W)) for i in range(12)]
    allc = ls + more
    sets = [PoseFromHeadGroupLaunch(allc[4 * k:4 * k + 4]) for k in range(4)]
    pipe = PnPPipeline(dev, depth=4, record_events=False)
    for k in range(8):
        pipe.submit(sets[k % 4], slot=k % 4)
    pipe.drain()
    ns = 24
    t0 = time.perf_counter()
    for k in range(ns):
        pipe.submit(sets[k % 4], slot=k % 4)
    pipe.drain()
    el = time.perf_counter() - t0
    same = all(bool(torch.equal(allc[4 + j].out['pose'], ls[j].out['pose']) and torch.equal(allc[4 + j].out['pose_cov_calib'], ls[j].out['pose_cov_calib'])) for j in range(4))
    out['in_flight_launch_sets'] = {'value': B_PER_GPU * 4 * ns / el, 'unit': 'solves/s', 'us_per_call': el / (4 * ns) * 1e6, 'launches_in_flight': pipe.depth,
                                    'calls_per_launch_set': 4, 'equal_the_calls_one_by_one': same}
    return out


def head_to_pose(torch, syn, PnPLaunch, dev, n_batches=4):
    """B = 1024 objects from the RAW NOC-head output (1024 x 30 x 28 x 28 fp32 = 96 MB per batch, 4 distinct resident batches =
    385 MB > the Infinity Cache; four = the depth of the pipeline the headline runs with) to poses: K2 alone (`noc_decode_kernel`, the one HBM-bound kernel of the path), K2 + PnP as two
    launches, and the fused one-launch kernel; each with its algorithmic bytes against the 8 TB/s HBM roofline."""
    from monorun_amd.pose_head import NocDecodeLaunch, PoseFromHeadLaunch, UncertPropPnPOptimizer, _planar_view, _clip_ranges
    head = UncertPropPnPOptimizer(pnp=dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False, initialiser='k0')).to(dev)      # the fast mode's one-launch head -> pose path
    k2s, fus, pnps = [], [], []
    for i in range(n_batches):
        b = syn.make_batch(B=B_PER_GPU, hw=HW, seed=SEED + 7919 * i)
        all_pred, dim = syn.encode_head_outputs(b, seed=SEED + i)
        rng = np.random.default_rng(SEED + i)
        dim_var = torch.from_numpy((0.01 * rng.random((B_PER_GPU, 3)) + 1e-4).astype(np.float32)).to(dev)      # MC-dropout variance of the dims (test time)
        ap, lab, dm, rois = (torch.from_numpy(all_pred).to(dev), torch.from_numpy(b['labels']).to(dev), torch.from_numpy(dim).to(dev),
                             torch.from_numpy(b['rois']).to(dev))
        K = torch.from_numpy(b['K']).to(dev)
        k2 = NocDecodeLaunch(ap, lab, False, dm, dim_var, rois)
        ur, vr = _clip_ranges((syn.IMG_H, syn.IMG_W), head.allowed_border, dev)
        d = k2.out
        pn = PnPLaunch(_planar_view(d['coords_2d']), _planar_view(d['coords_2d_istd']), _planar_view(d['coords_3d']), K, ur, vr, z_min=0.5,
                       epnp_istd_thres=0.6, epnp_ransac_thres=d['ransac_thr'], inlier_opt_only=True)
        fu = PoseFromHeadLaunch(head, ap, lab, False, dm, dim_var, rois, K, (syn.IMG_H, syn.IMG_W))
        k2s.append(k2); pnps.append(pn); fus.append(fu)
    px = B_PER_GPU * P
    bytes_k2 = px * (5 * 4 + 7 * 4) + B_PER_GPU * (20 + 24 + 8 + 12 + 12 + 4)
    bytes_fused = B_PER_GPU * (P * 5 * 4 + 20 + 24 + 8 + 16 + 64 + 4 + 1 + P + 64 + 12 + 12)
    t_k2 = graph_us_per_launch(torch, [k.run for k in k2s] * 4)
    t_two = graph_us_per_launch(torch, [f for k, q in zip(k2s, pnps) for f in (k.run, q.run)] * 2) * 2       # per (K2, PnP) pair
    t_fu = graph_us_per_launch(torch, [f.run for f in fus] * 2)
    # the two paths run the same device functions in the same order: identical results
    k2s[0].run(); pnps[0].run(); fus[0].run()
    torch.cuda.synchronize()
    same = bool(torch.equal(pnps[0].pose, fus[0].out['pose']) and torch.equal(pnps[0].mask, fus[0].out['inlier_mask_u8']))
    # the fused launches IN FLIGHT (the product's PnPPipeline, one slot per resident head output, the waves-per-object it asks for):
    # the regime of the headline, for the whole head -> pose path
    from monorun_amd import PnPPipeline
    pipe = PnPPipeline(dev, depth=n_batches, record_events=False)
    inflight = None
    if pipe.depth > 1:
        fl = pipe.flags_for(B_PER_GPU, P)
        fi = [PoseFromHeadLaunch(head, f.inputs['all_pred'], f.inputs['labels'], False, f.inputs['dim'], f.inputs['dim_var'], f.inputs['rois'],
                                 f.inputs['cam_intrinsic'] if 'cam_intrinsic' in f.inputs else K, (syn.IMG_H, syn.IMG_W), flags=fl) for f in fus[:pipe.depth]]
        for i in range(2 * len(fi)):
            pipe.submit(fi[i % len(fi)], slot=i % len(fi))
        pipe.drain()
        nrun = 48
        t1 = time.perf_counter()
        for i in range(nrun):
            pipe.submit(fi[i % len(fi)], slot=i % len(fi))
        pipe.drain()
        el = time.perf_counter() - t1
        ok = bool(torch.equal(fi[0].out['pose'], fus[0].out['pose']) and torch.equal(fi[0].out['inlier_mask_u8'], fus[0].out['inlier_mask_u8']))
        inflight = {'us_per_launch': el / nrun * 1e6, 'value': B_PER_GPU * nrun / el, 'unit': 'solves/s', 'launches_in_flight': len(fi),
                    'outputs_equal_the_one_stream_results': ok, 'roofline': roof_of(bytes_fused, el / nrun * 1e6)}
        del fi

    roof = roof_of
    return {
        'k2_noc_decode': {'us_per_launch': t_k2, 'value': B_PER_GPU / (t_k2 * 1e-6), 'unit': 'objects/s', 'roofline': roof(bytes_k2, t_k2),
                          'bytes_model': '48 B per RoI pixel (5 selected head channels read, 7 decoded channels written, fp32) + per-object vectors'},
        'two_launch': {'us_per_pair': t_two, 'value': B_PER_GPU / (t_two * 1e-6), 'unit': 'solves/s',
                       'roofline': roof(bytes_k2 + BYTES_PER_SOLVE * B_PER_GPU, t_two)},
        'fused': {'us_per_launch': t_fu, 'value': B_PER_GPU / (t_fu * 1e-6), 'unit': 'solves/s', 'roofline': roof(bytes_fused, t_fu),
                  'bytes_model': '20 B per RoI pixel read (the decoded maps never exist in HBM) + per-object inputs + pose / cov / calibrated cov / mask written'},
        'fused_in_flight': inflight,
        'fused_equals_two_launch': same,
        'how': f'{n_batches} distinct resident head outputs ({n_batches * B_PER_GPU * 30 * P * 4 / 2**20:.0f} MiB), launches captured into one HIP graph and replayed '
               '(no host latency between kernels); one stream, so the PnP launches pay their slowest object',
    }


def per_image_latency(torch, syn, dev, batch0, args, n_obj=100, calls=300, reference_flow=False):
    """B = 100 proposals of one image (monorun_roi_head.py:452: one image per forward; configs/kitti_car.py:200: max_per_img = 100): raw
    NOC-head output -> pose dict through the Python API (pose_from_head), eagerly, through a prepared launch (PoseFromHeadLaunch: arguments
    built once over static buffers) and as a HIP-graph replay of that launch.  reference_flow=False: the fast mode's head (ONE launch incl.
    decode, calibration, distance correction); True: the head as the reference's config dict builds it (K2 decode + the initialiser's launches +
    the re-fit / LM launch, monorun_roi_head.py:509-534).  wall_us_per_call_synced = host wall time per call with a stream synchronise after
    every call (what a per-image pipeline sees); issue_us_per_call = back-to-back enqueue cost."""
    from monorun_amd.pose_head import UncertPropPnPOptimizer, pose_from_head
    sub = {k: (v[:n_obj] if isinstance(v, np.ndarray) and v.shape[:1] == (batch0['labels'].shape[0],) else v) for k, v in batch0.items()}
    all_pred, dim = syn.encode_head_outputs(sub, seed=SEED)
    pnp_cfg = dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, forward_exact_hessian=False)      # configs/kitti_car.py:118-123
    if not reference_flow:
        pnp_cfg['initialiser'] = 'k0'                                   # the fast mode's one-launch head -> pose path
    head = UncertPropPnPOptimizer(pnp=pnp_cfg).to(dev)
    ap, lab, dm, rois = torch.from_numpy(all_pred).to(dev), torch.from_numpy(sub['labels']).to(dev), torch.from_numpy(dim).to(dev), torch.from_numpy(sub['rois']).to(dev)
    K = torch.from_numpy(sub['K']).to(dev)
    out = {}

    def call(**kw):
        with torch.no_grad():
            return pose_from_head(head, ap, lab, False, dm, None, rois, K, (syn.IMG_H, syn.IMG_W), **kw)
    from monorun_amd.pose_head import PoseFromHeadLaunch
    prepared = PoseFromHeadLaunch(head, ap, lab, False, dm, None, rois, K, (syn.IMG_H, syn.IMG_W))
    graph = PoseFromHeadLaunch(head, ap, lab, False, dm, None, rois, K, (syn.IMG_H, syn.IMG_W)).capture()
    variants = {'eager_pose_from_head': call, 'prepared_launch': prepared.run, 'hip_graph_replay': graph.replay}
    for name, fn in variants.items():
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(calls):
            fn()
            torch.cuda.current_stream().synchronize()
        wall = (time.perf_counter() - t1) / calls
        evs = [torch.cuda.Event() for _ in range(calls)]
        t1 = time.perf_counter()
        for e in evs:                                   # completion detected by polling an event instead of hipStreamSynchronize
            fn()
            e.record()
            while not e.query():
                pass
        spin = (time.perf_counter() - t1) / calls
        t1 = time.perf_counter()
        for _ in range(calls):
            fn()
        issue = (time.perf_counter() - t1) / calls
        torch.cuda.synchronize()
        thru = (time.perf_counter() - t1) / calls
        out[name] = {'wall_us_per_call_synced': wall * 1e6, 'wall_us_per_call_event_polled': spin * 1e6, 'issue_us_per_call': issue * 1e6,
                     'us_per_call_back_to_back': thru * 1e6}
    ref = call()
    for k in ('yaw_pred', 't_vec_pred', 'pose_cov_calib', 'inlier_mask'):      # the three paths are the same kernels on the same data
        assert torch.equal(prepared.out[k], graph.out[k]), k
        if reference_flow and k == 'pose_cov_calib':
            # the module path calibrates with three torch operations (uncert_prop_pnp_optimizer.py:96-97, monorun_roi_head.py:530-534), the prepared launches in the
            # LM launch's epilogue: the same float32 formula, exp from two libraries — equal to rounding
            assert torch.allclose(ref[k], prepared.out[k], rtol=2e-6, atol=0.0), k
        else:
            assert torch.equal(ref[k], prepared.out[k]), k
    out['objects'] = n_obj
    out['valid'] = int(ref['ret_val'].sum().item())
    out['outputs_of_the_three_paths_equal'] = True          # (the eager module path's calibrated covariance to 2e-6 relative in the reference flow: see above)
    # GPU time of one call: HIP events on the launch stream around prepared launches issued one at a time
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
    for e0, e1 in evs:
        e0.record(); prepared.run(); e1.record()
    torch.cuda.synchronize()
    out['gpu_us_per_call_hip_events'] = float(np.median([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3)
    return out


if __name__ == '__main__':
    main()
