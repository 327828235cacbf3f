"""The FLOP accounting bench.py reports against, pinned to SURVEY §8d / BASELINE.md §2."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_algorithmic_flops_match_survey():
    import Params
    b = _bench()
    net = Params.CTCParams.net_kernel_params
    total, fwd = b.step_flops(net, 256, 256, 4, 8)
    assert abs(fwd / 1e9 - 778.4) < 0.1                      # forward GFLOP/frame at config-2
    assert abs(total / 32 / 1e9 - 2266.6) < 0.2              # training GFLOP/frame
    assert abs(total / 1e12 - 72.53) < 0.01                  # TFLOP per step per GPU
    total4, fwd4 = b.step_flops(net, 832, 992, 2, 16)
    assert abs(fwd4 / 1e9 - 9803.6) < 1.0 and abs(total4 / 1e12 - 926.9) < 0.2     # config-4
    per_launch = b.lstm_step_flops(net, 256, 256, 4)
    assert [round(x / 1e9) for x in per_launch] == [866, 1288, 429, 322]
    assert b.PEAK_FP32_MFMA_TFLOPS == 157.3
    # the kernel-size variants of SURVEY D1 / §8d ("Variants at C2: all-5x5 -> 2 543.8; 3x3-LSTM -> 915.8 GFLOP/frame"; forward
    # 870.9 / 313.5) that `bench.py --net` and the `variants` block of the default line report
    t5, f5 = b.step_flops(b.net_by_name('default5'), 256, 256, 4, 8)
    t3, f3 = b.step_flops(b.net_by_name('lstm3'), 256, 256, 4, 8)
    assert abs(f5 / 1e9 - 870.9) < 0.1 and abs(t5 / 32 / 1e9 - 2543.8) < 0.2
    assert abs(f3 / 1e9 - 313.5) < 0.1 and abs(t3 / 32 / 1e9 - 915.8) < 0.2
    assert b.net_by_name('params') is Params.CTCParams.net_kernel_params


def test_bf16x3_lines_are_priced_against_the_bf16_peak():
    """Round-5 verdict, weak #6: no fraction of a peak above 1 on a 'bf16x3' line.  The mode's summary prices the bf16 MFMA FLOPs
    the pipe EXECUTES (6x the algorithmic FLOPs of the layers on split operands = sum over the bf16 kernel classes of rate x time)
    against the bf16 peak and reports the fp32-equivalent rate beside it; the committed line of the final set carries exactly that."""
    import json
    b = _bench()
    rows = [{'kernel': 'conv_halo_frag_kernel<5,LU_EPI_LSTM,*,bf16> (fused)', 'achieved': 1500.0, 'ms_per_step': 100.0},
            {'kernel': 'wgrad_row_x3_kernel<5> (bf16-MFMA ...)', 'achieved': 1600.0, 'ms_per_step': 90.0},
            {'kernel': 'conv_fwd_kernel (strided / dilated)', 'achieved': 100.0, 'ms_per_step': 10.0}]
    s = b.x3_summary(rows, 0.320, 72.53e12, 32)
    assert abs(s['executed_bf16_tflops'] - (1500.0 * 100 + 1600.0 * 90) / 320.0) < 0.1 and s['bf16_peak'] == 2500.0
    assert 0 < s['frac_of_bf16_peak'] < 1 and abs(s['fp32_equivalent_frames_per_s'] - 100.0) < 1e-6
    assert abs(s['algorithmic_fp32_tflops'] - 72.53 / 0.320) < 0.01 and not any('fp32_mfma_peak' in k for k in s)
    path = os.path.join(ROOT, 'profiles', 'r06_f32_bench_line.json')
    with open(path) as fh:
        line = [json.loads(l) for l in fh.read().splitlines() if l.startswith('{')][-1]

    def walk(o, where=''):
        if isinstance(o, dict):
            for k, v in o.items():
                if k.startswith('frac') and isinstance(v, (int, float)):
                    assert v <= 1.0, (where + '/' + k, v)
                walk(v, where + '/' + k)
        elif isinstance(o, list):
            for i, v in enumerate(o):
                walk(v, where + '[%d]' % i)
    walk(line)
    x3 = line['bf16x3_mode']
    assert x3['dtype'] == 'f32 results via 3 x bf16 split' and 'frac_of_fp32_mfma_peak' not in x3 and 'peak' not in x3
    assert line['dtype'] == 'f32' and 0.4 < x3['frac_of_bf16_peak'] < 0.7
    for v in line['variants'].values():
        assert 'frac_of_peak' not in v['bf16x3'] and v['bf16x3']['frac_of_bf16_peak'] < 1


def _start_bench(extra, env_extra):
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.Popen([sys.executable, os.path.join(ROOT, 'bench.py')] + extra, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _finish_bench(p, timeout=900):
    import json
    out, err = p.communicate(timeout=timeout)
    lines = [l for l in out.decode().splitlines() if l.startswith('{')]
    return p.returncode, (json.loads(lines[-1]) if lines else None), err.decode()[-3000:]


def _run_bench(extra, env_extra, timeout=900):
    import gpu_slots
    gpus = int(extra[extra.index('--gpus') + 1]) if '--gpus' in extra else 1
    launches = gpus > 1 and '--dry-run' not in extra and 'WORLD_SIZE' not in env_extra
    # bench.py itself, and when it self-launches: the torch.distributed.run agent and one process per rank
    with gpu_slots.hold(gpus + 2 if launches else 1):
        return _finish_bench(_start_bench(extra, env_extra), timeout)


def test_bench_refuses_mismatched_launches():
    """`--gpus N` must never print a one-GPU number under an N-GPU label: mismatches are exit code 2 (runs without a GPU)."""
    rc, line, err = _run_bench(['--gpus', '2'], {'WORLD_SIZE': '4', 'RANK': '0'})
    assert rc == 2 and line is None and 'WORLD_SIZE=4' in err
    rc, line, err = _run_bench(['--gpus', '0'], {})
    assert rc == 2 and line is None


SMALL = ['--steps', '2', '--warmup', '1', '--size', '64', '--batch', '1', '--unroll', '2', '--no-cpu-baseline', '--no-infer',
         '--no-bf16']


@pytest.mark.gpu
@pytest.mark.parametrize('backend', ['gloo', 'nccl'])
def test_bench_self_launches_n_ranks(backend):
    """`python bench.py --gpus 2` (no launcher) must start two ranks by itself and say what the collective layer saw.
    gloo: both ranks share the one GPU of the test box (control flow of the whole DP bench path on the HIP kernels);
    nccl (= RCCL): one device per rank; a box with fewer than two must refuse `--gpus 2`, and runs the RCCL path of the bench as
    a forced world of one instead (--force-collectives: process group, gradient buckets, loss sums and SyncBN statistics through
    real RCCL all-reduce calls on the one GPU)."""
    import torch
    if backend == 'nccl' and torch.cuda.device_count() < 2:
        rc, line, err = _run_bench(['--gpus', '2'] + SMALL, {'LU_DP_BACKEND': 'nccl'})
        assert rc == 2 and line is None and 'needs 2 visible GPUs' in err      # refuses instead of measuring one GPU
        rc, line, err = _run_bench(['--gpus', '1', '--sync-bn', '--force-collectives'] + SMALL, {'LU_DP_BACKEND': 'nccl'})
        assert rc == 0 and line is not None, err
        dp = line['dp']
        assert dp['backend'] == 'nccl' and dp['world_size'] == 1 and dp['forced_world_of_one'] and line['n_gpus'] == 1
        tr = dp['bucket_trace']
        assert tr and all(b['bytes'] > 0 for b in tr) and sum(b['bytes'] for b in tr) == sum(dp['gradient_bucket_bytes'])
        assert tr[0]['issued_ms_before_backward_end'] > 0 and dp['exposed_allreduce_ms'] is not None
        assert dp['allreduce_launches_per_step'] >= 1 and dp['allreduce_ms_per_step'] > 0 and dp['syncbn_allreduces_per_step'] == 32
        assert abs(line['value'] - 1 * 1 * 2 / (line['ms_per_step'] * 1e-3)) <= 0.01 * line['value']
        print('bench --gpus 1 --force-collectives over nccl: %s' % {k: dp[k] for k in dp if k != 'devices'})
        return
    rc, line, err = _run_bench(['--gpus', '2', '--sync-bn', '--check'] + SMALL, {'LU_DP_BACKEND': backend})
    assert rc == 0 and line is not None, err
    # --check: the DP == single-process comparison ran inline before the timing, and the overlap proof is on the line
    assert 'vs single process' in err and line['dp']['self_check']['ok'] and line['dp']['self_check']['grad_err_over_max'] <= 2e-6
    tr = line['dp']['bucket_trace']
    assert tr and all(b['bytes'] > 0 for b in tr) and sum(b['bytes'] for b in tr) == sum(line['dp']['gradient_bucket_bytes'])
    assert tr[0]['issued_ms_before_backward_end'] > 0      # the first bucket leaves while backward is still running
    assert line['dp']['exposed_allreduce_ms'] is not None
    assert line['n_gpus'] == 2 and line['config']['parallelism'] == 'dp2' and line['config']['global_batch'] == 2
    dp = line['dp']
    assert dp['world_size'] == 2 and dp['backend'] == backend and [d['rank'] for d in dp['devices']] == [0, 1]
    assert dp['distinct_devices'] == (1 if backend == 'gloo' else 2)
    assert dp['allreduce_launches_per_step'] >= 1 and dp['allreduce_ms_per_step'] > 0 and dp['syncbn_allreduces_per_step'] == 32
    assert line['metric'].endswith('at 64x64')
    # whole-job rate = all ranks' frames over the max-over-ranks time
    assert abs(line['value'] - 2 * 1 * 2 / (line['ms_per_step'] * 1e-3)) <= 0.01 * line['value']
    print('bench --gpus 2 over %s: %s' % (backend, {k: dp[k] for k in dp if k != 'devices'}))


def test_bench_dry_run_prints_the_rank_plan_without_a_gpu():
    """`bench.py --gpus 8 --dry-run`: validates devices / environment / port and prints the exact
    rank plan and gradient buckets without touching RCCL.  Here (no GPU): exit code 2 with the reason, and still the plan."""
    rc, line, err = _run_bench(['--gpus', '8', '--dry-run', '--sync-bn'], {})
    assert line is not None and line['dry_run'] and line['n_gpus'] == 8 and len(line['ranks']) == 8
    import torch
    if not torch.cuda.is_available():
        assert rc == 2 and not line['ok'] and any('no GPU visible' in p for p in line['problems'])
    assert [r['global_slots'] for r in line['ranks']][:2] == [[0, 1, 2, 3], [4, 5, 6, 7]] and line['config']['global_batch'] == 32
    assert [b['mbytes'] for b in line['gradient_buckets']] == [189.4, 101.2, 7.8]          # three buckets per step
    assert line['gradient_buckets'][0]['start'] == 0 and line['gradient_buckets'][-1]['end'] == line['parameters'] == 74606532
    assert line['collectives_per_step'] == {'gradient_all_reduce': 3, 'loss_sums_all_reduce': 1, 'sync_bn_all_reduce': 32}
    cmd = line['self_launch_command']
    assert '--nproc-per-node 8' in cmd and '--master-addr 127.0.0.1' in cmd and '--dry-run' not in cmd and '--gpus 8' in cmd
    assert line['self_launch_sets'] == {'HSA_ENABLE_IPC_MODE_LEGACY': '0'} or os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')
    # a launcher environment that disagrees with --gpus is named as a problem, like the real launch refuses it
    rc, line, err = _run_bench(['--gpus', '8', '--dry-run'], {'WORLD_SIZE': '4', 'RANK': '0'})
    assert rc == 2 and any('WORLD_SIZE=4' in p for p in line['problems']) and any('MASTER_PORT' in p for p in line['problems'])


@pytest.mark.gpu
def test_bench_dry_run_on_the_gpu_box():
    """On a box with fewer than 8 devices the RCCL plan is refused with the reason (exit code 2); the gloo plan (ranks sharing
    devices: control flow only) is accepted."""
    import torch
    n_dev = torch.cuda.device_count()
    rc, line, err = _run_bench(['--gpus', '8', '--dry-run'], {'LU_DP_BACKEND': 'gloo'})
    assert rc == 0 and line['ok'] and line['visible_devices'] == n_dev and line['backend'] == 'gloo', (line, err)
    assert [r['device'] for r in line['ranks']] == ['cuda:%d' % (r % n_dev) for r in range(8)]
    rc, line, err = _run_bench(['--gpus', '8', '--dry-run'], {'LU_DP_BACKEND': 'nccl'})
    if n_dev < 8:
        assert rc == 2 and any('one device per rank' in p for p in line['problems'])
    else:
        assert rc == 0 and line['ok']


def test_dump_outputs_sampling_is_fixed_and_within_budget(tmp_path):
    """`--dump-outputs`: float32 files, at most the byte budget in all, and a larger output replaced by the same sample every time."""
    import numpy as np
    import torch
    b = _bench()
    big = torch.arange(3 * 1000, dtype=torch.float32).view(10, 100, 3)
    arrays = {'softmax': big, 'loss': torch.tensor([0.5])}
    info = b.dump_outputs(str(tmp_path / 'a'), arrays, budget=4 * 1000)
    b.dump_outputs(str(tmp_path / 'b'), arrays, budget=4 * 1000)
    sizes = 0
    for name in arrays:
        a_, b_ = np.load(tmp_path / 'a' / (name + '.npy')), np.load(tmp_path / 'b' / (name + '.npy'))
        assert a_.dtype == np.float32 and np.array_equal(a_, b_)
        sizes += os.path.getsize(tmp_path / 'a' / (name + '.npy'))      # what lands on disk, headers included
    assert sizes <= 4 * 1000 and info['softmax']['sampled'] and info['loss']['sampled'] is None
    s = np.load(tmp_path / 'a' / 'softmax.npy')
    assert np.all(np.diff(s) > 0) and set(s.tolist()) <= set(big.view(-1).tolist())      # sorted positions of the real elements
    # under the budget: the arrays themselves, full shape
    b.dump_outputs(str(tmp_path / 'c'), arrays)
    assert np.array_equal(np.load(tmp_path / 'c' / 'softmax.npy'), big.numpy())


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_identically(tmp_path):
    """Two runs with the same arguments time exactly --steps steps and dump identical outputs of the last timed step."""
    import numpy as np
    args = ['--steps', '3', '--warmup', '1', '--size', '64', '--batch', '2', '--unroll', '2', '--no-cpu-baseline', '--no-infer',
            '--no-bf16', '--no-x3', '--no-variants']
    dumps = []
    for run in ('a', 'b'):
        rc, line, err = _run_bench(args + ['--dump-outputs', str(tmp_path / run)], {})
        assert rc == 0 and line is not None, err
        assert line['steps'] == 3 and line['ms_per_step'] > 0 and 'ms_per_step' in line
        assert set(line['dumped_outputs']) == {'softmax', 'predictions', 'loss'}
        dumps.append({n: np.load(tmp_path / run / (n + '.npy')) for n in line['dumped_outputs']})
    for n, a_ in dumps[0].items():
        assert a_.dtype == np.float32 and np.isfinite(a_).all() and np.array_equal(a_, dumps[1][n]), n
    assert sorted(dumps[0]['softmax'].shape) == [2, 2, 3, 64, 64] and dumps[0]['loss'].shape == (1,)
    assert sum(os.path.getsize(tmp_path / 'a' / (n + '.npy')) for n in dumps[0]) <= 64 * 2 ** 20
