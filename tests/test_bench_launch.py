"""The driver's launch contract: `python bench.py --gpus N ...` with NO launcher around it must start its N ranks itself (torch.distributed.run,
one process per GPU) -- here on the CPU tier: N = 2, the engine's host driver on the host simulator (OSQP_BENCH_HOSTSIM=1, a test-only switch
of bench.py), gloo.  Checks what a scaling run needs from the line: both ranks' records arrived, the sharded batch was solved by both ranks,
per-rank times are reported.  (The GPU-tier counterpart with RCCL is tests/test_gpu_rccl_one_rank.py.)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, extra):
    env = dict(os.environ, OSQP_BENCH_HOSTSIM='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)                                   # exactly the driver's situation: no launcher environment
    out = subprocess.run([sys.executable, os.path.join(ROOT, script)] + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]             # rank 0 prints ONE line
    return json.loads(lines[0])


def test_bench_starts_its_own_ranks():
    d = _run('bench.py', ['--gpus', '2', '--steps', '1', '--warmup', '0', '--vars', '300', '--batch', '6', '--batch-steps', '1', '--single-device', '--full'])
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and d['value'] > 0
    assert len(d['config']['per_rank']) == 2 and all(r['status'] == 1 for r in d['config']['per_rank'])
    assert d['config']['per_rank'][0]['iter'] == d['config']['per_rank'][1]['iter']          # replicas of one QP
    b = d['config']['batch']
    assert b['n_ranks_seen'] == 2 and b['solved'] == b['records'] == 6 and len(b['per_rank_ms']) == 2
    assert 'HOST SIMULATOR' in d['data'] and d['roofline'] is None                            # never mistaken for a measurement
    assert d['config']['solve_ms_hipevent_median'] is not None and d['config']['ms_per_step_median'] is not None


def test_single_rank_needs_no_launcher():
    d = _run('bench.py', ['--steps', '1', '--warmup', '0', '--vars', '300', '--batch', '4', '--batch-steps', '1', '--full'])
    assert d['n_gpus'] == 1 and d['config']['batch']['n_ranks_seen'] == 1 and d['config']['batch']['solved'] == 4


def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """A plain run (no --full): exactly --steps timed steps, ms_per_step in the line, nothing beyond the headline figure (no batch,
    no roofline, no CPU baseline); --dump-outputs writes x, y and info of the last timed step as float64, the same from run to run."""
    dumps = []
    for rep in range(2):
        out = tmp_path / ('run%d' % rep)
        d = _run('bench.py', ['--steps', '3', '--warmup', '1', '--vars', '300', '--dump-outputs', str(out)])
        assert d['steps'] == 3 and d['warmup'] == 1 and len(d['config']['admm_iters_per_step']) == 3
        assert d['ms_per_step'] > 0 and d['value'] > 0 and d['unit'] == 'ADMM iter/s' and d['higher_is_better'] is True and d['dtype'] == 'f64'
        assert 'batch' not in d['config'] and 'cpu_baseline' not in d and d['roofline'] is None and d['device'] is None
        files = {f.name: np.load(f) for f in out.iterdir()}
        assert set(files) == {'x.npy', 'y.npy', 'info.npy'}
        assert all(v.dtype == np.float64 for v in files.values()) and sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
        n, m = 300, 600
        assert files['x.npy'].shape == (n,) and files['y.npy'].shape == (m,)
        info = files['info.npy']
        assert info[0] == 1 and info[2] == d['config']['admm_iters_per_solve'] and info[4] == d['config']['obj_val']
        dumps.append(files)
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_dump_of_a_long_vector_is_a_fixed_sample(tmp_path):
    """A vector longer than bench.DUMP_MAX_ELEMS is written as the same seeded sample of its entries every time (in index order);
    four such vectors stay within 64 MB."""
    from types import SimpleNamespace
    sys.path.insert(0, ROOT)
    import bench
    k = bench.DUMP_MAX_ELEMS
    assert 4 * k * 8 < 64 << 20
    x = np.arange(2 * k + 7, dtype=np.float64)
    info = SimpleNamespace(**{f: 1.0 for f in bench.DUMP_INFO_FIELDS})
    res = SimpleNamespace(x=x, y=np.ones(5), prim_inf_cert=None, dual_inf_cert=None, info=info)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), res)
    xa, xb = np.load(tmp_path / 'a' / 'x.npy'), np.load(tmp_path / 'b' / 'x.npy')
    assert xa.shape == (k,) and np.array_equal(xa, xb) and np.all(np.diff(xa) > 0) and np.array_equal(np.load(tmp_path / 'a' / 'y.npy'), np.ones(5))
    assert np.load(tmp_path / 'a' / 'info.npy').shape == (len(bench.DUMP_INFO_FIELDS),)
