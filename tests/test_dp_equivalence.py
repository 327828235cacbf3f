"""N>1 path, world_size 2 over gloo on CPU (host-emulated kernels): one data-parallel training step with
SyncBN on two ranks x 1 slot must equal the single-process step on the 2-slot batch -- same loss, same
updated weights (loss sums all-reduced before the gradient, gradients SUMMED, BN statistics
pooled).  Also checks that rank-local BN (the fast mode) really differs, i.e. the switch does something."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gpu_slots
from conftest import tiny_net
from engine_backend import engine_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, 'lstm-unet_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np, torch
from engine_backend import engine_backend
from conftest import tiny_net
import train2D, Networks
from lu_native.dp import DataParallel
sync_bn = bool(int(sys.argv[1]))
with engine_backend('emu'):
    dp = DataParallel(backend='gloo')
    d = np.load(os.path.join(%(tmp)r, 'batch.npz'))
    tr = train2D.Trainer(Networks.ULSTMnet2D, tiny_net(3), 'NHWC', [0.15, 0.25, 0.6], 1e-3, dp=dp, sync_bn=sync_bn, seed=3)
    sl = slice(dp.rank, dp.rank + 1)
    _, _, loss = tr.train_step(d['x'][sl], d['gt'][sl])
    grads1 = tr.engine.flat_grads.numpy().copy()          # all-reduced, before Adam touches anything
    tr.model.reset_states_per_batch(np.ones(1, np.float32))
    _, _, loss2 = tr.train_step(d['x'][sl, ::-1].copy(), d['gt'][sl, ::-1].copy())
    if dp.rank == 0:
        np.savez(os.path.join(%(tmp)r, 'dp_out_%%d.npz' %% int(sync_bn)), params=tr.engine.flat_params.numpy(),
                 loss=np.array([float(loss), float(loss2)]), grads1=grads1)
    dp.barrier()
'''


def test_dp2_equals_single_process(tmp_path):
    import train2D
    import Networks
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 2, 16, 16, 1)).astype(np.float32)
    gt = rng.integers(-1, 3, size=(2, 2, 16, 16, 1)).astype(np.float32)
    np.savez(tmp_path / 'batch.npz', x=x, gt=gt)
    script = tmp_path / 'worker.py'
    script.write_text(WORKER % {'root': ROOT, 'tmp': str(tmp_path)})
    for sync_bn in (1, 0):
        port = 29600 + (os.getpid() + sync_bn) % 1500
        with gpu_slots.hold(2):
            procs = [subprocess.Popen([sys.executable, str(script), str(sync_bn)],
                                      env=dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r),
                                               MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port)),
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
            outs = [p.communicate(timeout=900)[0].decode() for p in procs]
        for p, o in zip(procs, outs):
            assert p.returncode == 0, o[-3000:]
    with engine_backend('emu'):
        tr = train2D.Trainer(Networks.ULSTMnet2D, tiny_net(3), 'NHWC', [0.15, 0.25, 0.6], 1e-3, seed=3)
        _, _, l1 = tr.train_step(x, gt)
        ref_grads1 = tr.engine.flat_grads.numpy().copy()
        tr.model.reset_states_per_batch(np.ones(2, np.float32))
        _, _, l2 = tr.train_step(x[:, ::-1].copy(), gt[:, ::-1].copy())
        ref = tr.engine.flat_params.numpy().copy()
        ref_loss = np.array([float(l1), float(l2)])
    sync = np.load(tmp_path / 'dp_out_1.npz')
    local = np.load(tmp_path / 'dp_out_0.npz')
    assert np.abs(sync['loss'] - ref_loss).max() <= 1e-5, (sync['loss'], ref_loss)
    # the all-reduced GRADIENTS of step 1 (pre-Adam: a wrong scale on any bucket shows here, Adam would normalise it away)
    g_err = np.abs(sync['grads1'] - ref_grads1).max() / np.abs(ref_grads1).max()
    print('dp2 vs single, step-1 gradients: max err / max|g| = %.3e' % g_err)
    assert g_err <= 1e-6, g_err
    for name, s_, e_ in tr.engine.segments:               # ... and per bucket, relative to the bucket's own scale
        ref_b, got_b = ref_grads1[s_:e_], sync['grads1'][s_:e_]
        assert np.abs(got_b - ref_b).max() <= 1e-5 * max(np.abs(ref_b).max(), 1e-30), name
    # Adam normalises the step size, so compare weights loosely in count and tightly in the bulk
    diff = np.abs(sync['params'] - ref)
    assert diff.max() <= 2.5e-3 and (diff > 1e-4).mean() <= 2e-3, (diff.max(), (diff > 1e-4).mean())
    # rank-local BN is a different (documented) model: it must NOT coincide with the pooled statistics
    assert np.abs(local['loss'] - ref_loss).max() > 1e-6


GPU_WORKER = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, 'lstm-unet_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np, torch
from conftest import tiny_net
import train2D, Networks
from lu_native.dp import DataParallel
dp = DataParallel(bucket_bytes=int(os.environ.get('LU_TEST_BUCKET_BYTES', 64 << 20)))      # LU_DP_BACKEND=gloo: all ranks on the ONE GPU of the box, HIP kernels underneath
assert dp.world_size == int(os.environ['WORLD_SIZE']) and torch.cuda.is_available()
assert list(dp.shard_slots(dp.world_size)) == [dp.rank] and list(dp.shard_slots(2 * dp.world_size)) == [2 * dp.rank, 2 * dp.rank + 1]
d = np.load(os.path.join(%(tmp)r, 'batch.npz'))
net = tiny_net(3, (64, 16, 16, 64), (16, 8, 8, 8)) if sys.argv[1] == 'bf16x3' else tiny_net(3, (32, 16, 16, 32), (16, 8, 8, 8))
tr = train2D.Trainer(Networks.ULSTMnet2D, net, 'NCHW', [0.15, 0.25, 0.6], 1e-3, dp=dp, sync_bn=True, seed=3,
                     precision=sys.argv[1])
if os.environ.get('LU_TEST_NO_OVERLAP'):
    tr.engine.overlap_wgrad = False
sl = slice(dp.rank, dp.rank + 1)
_, _, loss = tr.train_step(d['x'][sl], d['gt'][sl])
grads1 = tr.engine.flat_grads.cpu().numpy()
tr.model.reset_states_per_batch(np.ones(1, np.float32))
_, _, loss2 = tr.train_step(d['x'][sl, ::-1].copy(), d['gt'][sl, ::-1].copy())
torch.cuda.synchronize()
if dp.rank == 0:
    np.savez(os.path.join(%(tmp)r, 'dp_gpu_out.npz'), params=tr.engine.flat_params.cpu().numpy(),
             loss=np.array([float(loss), float(loss2)]), grads1=grads1, launched=np.array([dp.launched]),
             ranges=np.array(dp.last_ranges))
dp.barrier()
'''


def _launch_dp2(tmp_path, precision):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 3, 1, 24, 32)).astype(np.float32)
    gt = rng.integers(-1, 3, size=(2, 3, 1, 24, 32)).astype(np.float32)
    np.savez(tmp_path / 'batch.npz', x=x, gt=gt)
    script = tmp_path / 'worker_gpu.py'
    script.write_text(GPU_WORKER % {'root': ROOT, 'tmp': str(tmp_path)})
    port = 29600 + (os.getpid() + 11 * ['fp32', 'bf16', 'bf16x3'].index(precision)) % 1500      # (the three may be in flight at once)
    procs = [subprocess.Popen([sys.executable, str(script), precision],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK='0', LU_DP_BACKEND='gloo',
                                       MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    return {'tmp': tmp_path, 'procs': procs, 'x': x, 'gt': gt}


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
def test_dp2_syncbn_on_the_hip_kernels_equals_single_process(tmp_path, precision):
    """The N > 1 path on the REAL kernels: two ranks (gloo, sharing the one GPU of the test box -- RCCL needs one device
    per rank) x 1 slot with SyncBN == one process on the 2-slot batch.  What runs: rank-sharded slots, loss-sum all-reduce
    before the gradient, bucketed gradient all-reduce fired from the engine's backward, pooled BN statistics.
    precision='bf16': the engine then runs its weight gradients on the side stream, so every bucket hand-over has to join
    it first (LU_TEST_NO_OVERLAP=1 runs the same comparison with the side stream off).
    precision='bf16x3' (on a net whose first and last ConvLSTM layers, F = 64, take the split route): fp32 arithmetic, so the fp32
    limits apply -- gradients to summation-order noise."""
    import train2D
    import Networks
    with gpu_slots.hold(2):
        h = _launch_dp2(tmp_path, precision)
        tmp_path, procs, x, gt = h['tmp'], h['procs'], h['x'], h['gt']
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    net = tiny_net(3, (64, 16, 16, 64), (16, 8, 8, 8)) if precision == 'bf16x3' else tiny_net(3, (32, 16, 16, 32), (16, 8, 8, 8))
    tr = train2D.Trainer(Networks.ULSTMnet2D, net, 'NCHW', [0.15, 0.25, 0.6], 1e-3, seed=3, precision=precision)
    if os.environ.get('LU_TEST_NO_OVERLAP'):
        tr.engine.overlap_wgrad = False
    _, _, l1 = tr.train_step(x, gt)
    ref_grads1 = tr.engine.flat_grads.cpu().numpy()
    tr.model.reset_states_per_batch(np.ones(2, np.float32))
    _, _, l2 = tr.train_step(x[:, ::-1].copy(), gt[:, ::-1].copy())
    ref = tr.engine.flat_params.cpu().numpy()
    got = np.load(tmp_path / 'dp_gpu_out.npz')
    assert np.abs(got['loss'] - np.array([float(l1), float(l2)])).max() <= 1e-5
    # pre-Adam all-reduced gradients of step 1: fp32 to summation-order noise; bf16 mode re-rounds a few activations
    # (pooled-vs-whole-batch statistics differ in the last bits), stated 2e-3 of the largest gradient
    g_err = np.abs(got['grads1'] - ref_grads1).max() / np.abs(ref_grads1).max()
    print('dp2 vs single (%s), step-1 gradients: max err / max|g| = %.3e' % (precision, g_err))
    assert g_err <= (2e-3 if precision == 'bf16' else 2e-6), g_err
    diff = np.abs(got['params'] - ref)
    print('dp2 vs single (%s): max %.3e, fraction > 1e-4: %.3e' % (precision, diff.max(), (diff > 1e-4).mean()))
    # bf16: the two wide ConvLSTM layers of this net (4F = 128 columns) do run on the bf16 MFMA kernels; pooled-vs-whole-batch
    # BN statistics differ in the last fp64 bits, a few activations then round to the other bf16 neighbour, and Adam turns
    # that into 1e-4-sized steps on ~0.5 % of the weights (measured 1.06e-3 / 5.2e-3, identical with the side stream off)
    # (round 3: the narrow decoder layers round to bf16 as well: 2.4e-2 of the weights; the pre-Adam gradients above are the
    # sharp check -- 8.7e-5 of the largest gradient)
    frac = 5e-2 if precision == 'bf16' else 2e-3
    assert diff.max() <= 2.5e-3 and (diff > 1e-4).mean() <= frac, (diff.max(), (diff > 1e-4).mean())


# ranks that share the one GPU of the test box: with the pytest process itself, at most six processes hold the GPU at once
ONE_GPU_RANKS = 5


def _launch_dp5_syncbn(tmp_path):
    W = ONE_GPU_RANKS
    rng = np.random.default_rng(8)
    x = rng.standard_normal((W, 3, 1, 24, 32)).astype(np.float32)
    gt = rng.integers(-1, 3, size=(W, 3, 1, 24, 32)).astype(np.float32)
    np.savez(tmp_path / 'batch.npz', x=x, gt=gt)
    script = tmp_path / 'worker_gpu.py'
    script.write_text(GPU_WORKER % {'root': ROOT, 'tmp': str(tmp_path)})
    port = 29600 + (os.getpid() + 333) % 1500
    procs = [subprocess.Popen([sys.executable, str(script), 'fp32'],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(W), LOCAL_RANK='0', LU_DP_BACKEND='gloo',
                                       LU_TEST_BUCKET_BYTES='65536', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(W)]
    return {'tmp': tmp_path, 'procs': procs, 'x': x, 'gt': gt}


@pytest.mark.gpu
def test_dp5_syncbn_three_buckets_over_gloo_on_one_gpu_equals_single_process(tmp_path):
    """FIVE ranks x 1 slot on the real kernels (gloo, all on the one GPU of the test box): shard_slots
    with W = 5 (not a power of two), SyncBN with 5 contributors, the gradient all-reduce in THREE OR MORE buckets (a small bucket
    size: the tiny net's 0.1 MB of gradients would otherwise leave as one), loss sums over 5 ranks -- loss and pre-Adam
    gradients must equal the single-process step on the 5-slot batch.  Five, not eight: with the pytest process, six processes
    hold the one GPU, the most a shared box allows.  What a multi-GPU box adds to this is RCCL itself and one device per rank."""
    import train2D
    import Networks
    W = ONE_GPU_RANKS
    with gpu_slots.hold(W):
        h = _launch_dp5_syncbn(tmp_path)
        tmp_path, procs, x, gt = h['tmp'], h['procs'], h['x'], h['gt']
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    net = tiny_net(3, (32, 16, 16, 32), (16, 8, 8, 8))
    tr = train2D.Trainer(Networks.ULSTMnet2D, net, 'NCHW', [0.15, 0.25, 0.6], 1e-3, seed=3)
    _, _, l1 = tr.train_step(x, gt)
    ref_grads1 = tr.engine.flat_grads.cpu().numpy()
    tr.model.reset_states_per_batch(np.ones(W, np.float32))
    _, _, l2 = tr.train_step(x[:, ::-1].copy(), gt[:, ::-1].copy())
    got = np.load(tmp_path / 'dp_gpu_out.npz')
    g_err = np.abs(got['grads1'] - ref_grads1).max() / np.abs(ref_grads1).max()
    ranges = got['ranges']
    print('dp%d over gloo on one GPU vs single: loss err %.3e, step-1 gradient err / max|g| %.3e, %d buckets %s' %
          (W, np.abs(got['loss'] - np.array([float(l1), float(l2)])).max(), g_err, len(ranges), ranges.tolist()))
    assert np.abs(got['loss'] - np.array([float(l1), float(l2)])).max() <= 1e-5 and g_err <= 2e-6
    # buckets: at least three, contiguous, covering the flat gradient buffer front to back (backward-completion order)
    assert len(ranges) >= 3 and ranges[0][0] == 0 and ranges[-1][1] == tr.engine.n_flat
    assert all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))


RCCL_WORKER = r'''
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, 'lstm-unet_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np, torch
from conftest import tiny_net
import train2D, Networks
from lu_native.dp import DataParallel
dp = DataParallel(backend='nccl', force=True)       # RCCL: one device per rank (LOCAL_RANK); a world of one still all-reduces
assert dp.collectives and dp.world_size == int(os.environ['WORLD_SIZE'])
assert torch.distributed.get_backend() == 'nccl' and torch.cuda.current_device() == dp.local_rank
d = np.load(os.path.join(%(tmp)r, 'batch.npz'))
net = tiny_net(3, (32, 16, 16, 32), (16, 8, 8, 8))
tr = train2D.Trainer(Networks.ULSTMnet2D, net, 'NCHW', [0.15, 0.25, 0.6], 1e-3, dp=dp, sync_bn=True, seed=3,
                     precision=sys.argv[1])
per = d['x'].shape[0] // dp.world_size
sl = slice(dp.rank * per, (dp.rank + 1) * per)
_, _, loss = tr.train_step(d['x'][sl], d['gt'][sl])
grads1 = tr.engine.flat_grads.cpu().numpy()
tr.model.reset_states_per_batch(np.ones(per, np.float32))
_, _, loss2 = tr.train_step(d['x'][sl, ::-1].copy(), d['gt'][sl, ::-1].copy())
torch.cuda.synchronize()
if dp.rank == 0:
    np.savez(os.path.join(%(tmp)r, 'dp_rccl_out.npz'), params=tr.engine.flat_params.cpu().numpy(),
             loss=np.array([float(loss), float(loss2)]), grads1=grads1, launched=np.array([dp.launched]))
dp.barrier()
torch.distributed.destroy_process_group()
'''


@pytest.mark.gpu
def test_dp_syncbn_over_rccl_one_rank_per_device_equals_single_process(tmp_path):
    """The self-check for a multi-GPU box: N ranks, one device each, backend nccl (= RCCL over xGMI), SyncBN: loss and pre-Adam
    gradients must equal the single-process step on the N-slot batch (fp32: summation-order noise).  N = every visible device, at
    most ONE_GPU_RANKS (with pytest, six processes hold GPUs).  RCCL refuses two ranks on one device, so a one-GPU box runs N = 1
    with the collectives forced on: the process group, the gradient buckets, the loss sums and the SyncBN statistics still go
    through real RCCL all-reduce calls (the N-rank control flow on one GPU: the gloo tests above)."""
    n_ranks = max(1, min(torch.cuda.device_count(), ONE_GPU_RANKS))
    import train2D
    import Networks
    rng = np.random.default_rng(n_ranks)
    x = rng.standard_normal((n_ranks, 3, 1, 24, 32)).astype(np.float32)
    gt = rng.integers(-1, 3, size=(n_ranks, 3, 1, 24, 32)).astype(np.float32)
    np.savez(tmp_path / 'batch.npz', x=x, gt=gt)
    script = tmp_path / 'worker_rccl.py'
    script.write_text(RCCL_WORKER % {'root': ROOT, 'tmp': str(tmp_path)})
    port = 29600 + (os.getpid() + 7 * n_ranks) % 1500
    env = {k: v for k, v in os.environ.items() if k != 'LU_DP_BACKEND'}
    with gpu_slots.hold(n_ranks):
        procs = [subprocess.Popen([sys.executable, str(script), 'fp32'],
                                  env=dict(env, RANK=str(r), WORLD_SIZE=str(n_ranks), LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1',
                                           MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0'),
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(n_ranks)]
        outs = [p.communicate(timeout=900)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    net = tiny_net(3, (32, 16, 16, 32), (16, 8, 8, 8))
    tr = train2D.Trainer(Networks.ULSTMnet2D, net, 'NCHW', [0.15, 0.25, 0.6], 1e-3, seed=3)
    _, _, l1 = tr.train_step(x, gt)
    ref_grads1 = tr.engine.flat_grads.cpu().numpy()
    tr.model.reset_states_per_batch(np.ones(n_ranks, np.float32))
    _, _, l2 = tr.train_step(x[:, ::-1].copy(), gt[:, ::-1].copy())
    got = np.load(tmp_path / 'dp_rccl_out.npz')
    g_err = np.abs(got['grads1'] - ref_grads1).max() / np.abs(ref_grads1).max()
    print('dp%d over RCCL vs single: loss err %.3e, step-1 gradient err / max|g| %.3e, all-reduce launches %d' %
          (n_ranks, np.abs(got['loss'] - np.array([float(l1), float(l2)])).max(), g_err, int(got['launched'][0])))
    assert np.abs(got['loss'] - np.array([float(l1), float(l2)])).max() <= 1e-5 and g_err <= 2e-6
    assert int(got['launched'][0]) >= 2                     # gradient buckets of both steps went through RCCL


FORCED_WORKER = r"""
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, 'lstm-unet_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np, torch
from conftest import tiny_net
import train2D, Networks
from lu_native.dp import DataParallel
forced = sys.argv[2] == 'forced'
dp = DataParallel(backend='nccl', bucket_bytes=8 << 10, force=True) if forced else DataParallel.solo()
if forced:
    import torch.distributed as dist
    assert dp.collectives and dp.world_size == 1 and dist.is_initialized() and dist.get_backend() == 'nccl' and dist.get_world_size() == 1
d = np.load(os.path.join(%(tmp)r, 'batch.npz'))
net = tiny_net(3, (32, 16, 16, 32), (16, 8, 8, 8))
tr = train2D.Trainer(Networks.ULSTMnet2D, net, 'NCHW', [0.15, 0.25, 0.6], 1e-3, dp=dp, sync_bn=forced, seed=3, precision=sys.argv[1])
assert tr.engine.sync_bn == forced
if forced:
    dp.trace = []
_, _, loss = tr.train_step(d['x'], d['gt'])
grads1 = tr.engine.flat_grads.cpu().numpy()
tr.model.reset_states_per_batch(np.ones(d['x'].shape[0], np.float32))
_, _, loss2 = tr.train_step(d['x'][:, ::-1].copy(), d['gt'][:, ::-1].copy())
torch.cuda.synchronize()
trace = dp.trace_report() if forced else []
np.savez(os.path.join(%(tmp)r, 'dp1_%%s.npz' %% sys.argv[2]), params=tr.engine.flat_params.cpu().numpy(), loss=np.array([float(loss), float(loss2)]),
         grads1=grads1, grads2=tr.engine.flat_grads.cpu().numpy(), launched=np.array([dp.launched]),
         ranges=np.array(dp.last_ranges).reshape(-1, 2), n_flat=np.array([tr.engine.n_flat]),
         librccl=np.array([int(any('librccl' in l for l in open('/proc/self/maps')))]),
         issued=np.array([b['issued_ms_before_backward_end'] for b in (trace[-1] if trace else [])]))
if forced:
    dp.barrier()
    torch.distributed.destroy_process_group()
"""


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_dp1_rccl_forced_collectives_equals_plain_step(tmp_path, precision):
    """RCCL with the hardware that exists: ONE rank.  DataParallel(force=True) (LU_DP_FORCE=1, bench.py --force-collectives)
    initialises backend 'nccl' with WORLD_SIZE = 1 and sends every gradient bucket (async handles, waited for in finish()), the
    loss sums and the SyncBN statistics through real ncclAllReduce calls on the one GPU -- the stream ordering between the compute
    stream, the weight-gradient side stream (bf16) and RCCL's stream, the async-handle semantics gloo does not have and the
    flat-buffer slicing; everything of SURVEY 8e's step except the wire.  A sum over one rank is the identity: two training
    steps must give BIT-IDENTICAL losses, gradients and Adam-updated parameters to the plain single-process step."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 3, 1, 24, 32)).astype(np.float32)
    gt = rng.integers(-1, 3, size=(2, 3, 1, 24, 32)).astype(np.float32)
    np.savez(tmp_path / 'batch.npz', x=x, gt=gt)
    script = tmp_path / 'worker_forced.py'
    script.write_text(FORCED_WORKER % {'root': ROOT, 'tmp': str(tmp_path)})
    port = 29600 + (os.getpid() + 13) % 1500
    env = {k: v for k, v in os.environ.items() if k not in ('LU_DP_BACKEND', 'LU_DP_FORCE', 'RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    for mode in ('forced', 'plain'):
        with gpu_slots.hold(1):
            p = subprocess.run([sys.executable, str(script), precision, mode],
                               env=dict(env, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0'),
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert p.returncode == 0, p.stdout.decode()[-3000:]
    a, b = np.load(tmp_path / 'dp1_forced.npz'), np.load(tmp_path / 'dp1_plain.npz')
    ranges = a['ranges']
    print('dp1 forced over RCCL [%s]: %d all-reduce launches in two steps, buckets of the last step %s, handed over %s ms before the end '
          'of backward; librccl mapped: forced %d / plain %d' % (precision, int(a['launched'][0]), ranges.tolist(),
                                                                 np.round(a['issued'], 3).tolist(), int(a['librccl'][0]), int(b['librccl'][0])))
    assert int(a['librccl'][0]) == 1 and int(b['launched'][0]) == 0
    # at least three buckets per step, contiguous, covering the flat gradient buffer front to back (backward-completion order)
    assert int(a['launched'][0]) >= 6 and len(ranges) >= 3 and ranges[0][0] == 0 and ranges[-1][1] == int(a['n_flat'][0])
    assert all(ranges[i][1] == ranges[i + 1][0] for i in range(len(ranges) - 1))
    for k in ('loss', 'grads1', 'grads2', 'params'):
        assert np.array_equal(a[k], b[k]), k


FORCED_GLOO_WORKER = r"""
import os, sys
ROOT = %(root)r
for p in (ROOT, os.path.join(ROOT, 'lstm-unet_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import numpy as np, torch
from engine_backend import engine_backend
from conftest import tiny_net
import train2D, Networks
from lu_native.dp import DataParallel
out = {}
with engine_backend('emu'):
    d = np.load(os.path.join(%(tmp)r, 'batch.npz'))
    for mode in ('forced', 'plain'):
        dp = DataParallel(backend='gloo', bucket_bytes=1 << 10, force=True) if mode == 'forced' else DataParallel.solo()
        tr = train2D.Trainer(Networks.ULSTMnet2D, tiny_net(3), 'NHWC', [0.15, 0.25, 0.6], 1e-3, dp=dp, sync_bn=(mode == 'forced'), seed=3)
        assert tr.engine.sync_bn == (mode == 'forced') and dp.collectives == (mode == 'forced')
        _, _, loss = tr.train_step(d['x'], d['gt'])
        out[mode + '_grads'] = tr.engine.flat_grads.numpy().copy()
        out[mode + '_loss'] = np.array([float(loss)])
        out[mode + '_launched'] = np.array([dp.launched])
        out[mode + '_ranges'] = np.array(dp.last_ranges).reshape(-1, 2)
        out['n_flat'] = np.array([tr.engine.n_flat])
    assert torch.distributed.is_initialized() and torch.distributed.get_world_size() == 1
    np.savez(os.path.join(%(tmp)r, 'dp1_gloo.npz'), **out)
    torch.distributed.destroy_process_group()
"""


def test_dp1_forced_collectives_over_gloo_equals_plain_step(tmp_path):
    """The control flow of DataParallel(force=True) -- a world of ONE that still initialises the process group and routes the
    gradient buckets, loss sums and SyncBN statistics through all-reduce calls -- on the host-emulated kernels over gloo
    (the RCCL leg: test_dp1_rccl_forced_collectives_equals_plain_step, -m gpu).  Identity sums: bit-identical to the plain step."""
    rng = np.random.default_rng(5)
    np.savez(tmp_path / 'batch.npz', x=rng.standard_normal((1, 2, 16, 16, 1)).astype(np.float32),      # (one slot: the emulator is slow)
             gt=rng.integers(-1, 3, size=(1, 2, 16, 16, 1)).astype(np.float32))
    script = tmp_path / 'worker_forced_gloo.py'
    script.write_text(FORCED_GLOO_WORKER % {'root': ROOT, 'tmp': str(tmp_path)})
    env = {k: v for k, v in os.environ.items() if k not in ('LU_DP_BACKEND', 'LU_DP_FORCE', 'RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    with gpu_slots.hold(1):
        p = subprocess.run([sys.executable, str(script)], env=dict(env, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(29600 + (os.getpid() + 29) % 1500)),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    d = np.load(tmp_path / 'dp1_gloo.npz')
    r = d['forced_ranges']
    assert int(d['plain_launched'][0]) == 0 and int(d['forced_launched'][0]) == len(r) >= 3
    assert r[0][0] == 0 and r[-1][1] == int(d['n_flat'][0]) and all(r[i][1] == r[i + 1][0] for i in range(len(r) - 1))
    assert np.array_equal(d['forced_grads'], d['plain_grads']) and np.array_equal(d['forced_loss'], d['plain_loss'])
