"""Distributed fused engine on ONE GPU: 2 ranks over gloo (RCCL forbids two ranks per device), both on
cuda:0.  Checks that the SyncBN exchange + bucketed gradient all-reduce of the fused step reproduce a
single-process step on the concatenated batch."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ['ROOT'])
from medical_segmentation_pytorch_amd.models.ducknet import DuckNet
from medical_segmentation_pytorch_amd.runtime.trainer_engine import FusedStep
dist.init_process_group('gloo')
rank, world = dist.get_rank(), dist.get_world_size()
dev = torch.device('cuda', 0)
torch.manual_seed(0)
model = DuckNet(2, 3, 8).to(dev).train()
g = torch.Generator().manual_seed(1)
x = torch.randn(4, 3, 128, 128, generator=g).to(dev)   # the global batch, same for every world size
# labels correlated with the input (random per-pixel labels give a gradient that is a heavily
# cancelling sum of noise, which amplifies bf16 rounding differences beyond any useful tolerance)
y = (torch.nn.functional.avg_pool2d(x[:, :1], 9, 1, 4)[:, 0] > 0).long().to(dev)
if os.environ.get('PERTURB') == '1':   # noise-floor run: bf16-rounding-sized input perturbation
    x = x * (1 + 4e-3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev))
if world == 1 or os.environ.get('DUP') == '1':   # DUP: every rank holds the full batch
    xs, ys = x, y
else:
    xs, ys = x[2 * rank:2 * rank + 2].contiguous(), y[2 * rank:2 * rank + 2].contiguous()
w0 = [p.detach().float().cpu().clone() for p in model.parameters()]
names = [n for n, _ in model.named_parameters()]
step = FusedStep(model, xs, ys, optimizer='sgd', lr=0.05, momentum=0.0, use_graph=False,
                 distributed=world > 1, syncbn=True, bucket_cap_mb=0.5)
step.sched.max_lr = 0.05
from medical_segmentation_pytorch_amd.ops import bn as bnmod
ex0 = bnmod.EXCHANGES[0]
loss = step()
torch.cuda.synchronize()
exchanges = bnmod.EXCHANGES[0] - ex0
n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules())
loss = torch.tensor([float(loss)])
dist.all_reduce(loss)                     # mean of the per-rank half-batch losses == full-batch loss
loss = loss / world
if rank == 0:
    upd = [p.detach().float().cpu() - a for p, a in zip(model.parameters(), w0)]   # the SGD update
    w = torch.cat([u.flatten() for u in upd])
    rms = [b.detach().float().cpu() for n, b in model.named_buffers() if 'running_mean' in n]
    from medical_segmentation_pytorch_amd.runtime import comm
    torch.save({'w': w, 'upd': upd, 'names': names, 'rm': torch.cat(rms), 'rms': rms, 'loss': float(loss),
                'exchanges': exchanges, 'n_bn': n_bn, 'path': comm.describe()}, os.environ['OUT'])
dist.destroy_process_group()
'''


def _run(world, out, tmp, dup=False, perturb=False, syncbn_comm='auto'):
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    script = tmp / 'w.py'
    script.write_text(WORKER)
    env = dict(os.environ, ROOT=ROOT, OUT=str(out), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
               DUP='1' if dup else '0', PERTURB='1' if perturb else '0', MSP_SYNCBN_COMM=syncbn_comm)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out, weights_only=True)


def test_replicated_batch_is_exact(gpu, tmp_path):
    """Both ranks hold the SAME full batch: SyncBN statistics and averaged gradients are then
    mathematically identical to the single-process step, so only rounding may differ -- this isolates
    exchange bugs from the bf16 drift of the split-batch comparison below."""
    one = _run(1, tmp_path / 'one.pt', tmp_path)
    dup = _run(2, tmp_path / 'dup.pt', tmp_path, dup=True)
    per = sorted(((((a - b).norm() / a.norm().clamp_min(1e-20)).item(), (b.norm() / a.norm().clamp_min(1e-20)).item(), n)
                  for a, b, n in zip(one['upd'], dup['upd'], one['names'])), reverse=True)
    print('replicated: worst params (rel diff, norm ratio, name):', per[:8])
    rel = [((a - b).norm() / a.norm().clamp_min(1e-12)).item() for a, b in zip(one['rms'], dup['rms'])]
    print('replicated: max running_mean rel diff', max(rel))
    assert max(rel) < 1e-4, rel
    assert per[0][0] < 1e-2, per[:8]


def test_syncbn_ipc_exchange_bitwise_equals_collective(gpu, tmp_path):
    """The SyncBN exchange on the IPC peer-memory kernel vs the process group's collective (gloo here: RCCL
    refuses two ranks on one GPU): with two ranks both sum x0 + x1 in fp64, so the whole training step --
    statistics, data-gradients, the averaged update -- must be BITWISE identical."""
    ipc = _run(2, tmp_path / 'ipc.pt', tmp_path, syncbn_comm='ipc')
    col = _run(2, tmp_path / 'col.pt', tmp_path, syncbn_comm='rccl')
    assert ipc['path'] == ['ipc'] and col['path'] == ['rccl'], (ipc['path'], col['path'])
    assert ipc['exchanges'] == col['exchanges'] > 0
    assert torch.equal(ipc['rm'], col['rm'])
    assert torch.equal(ipc['w'], col['w'])


def _upd_rel(a, b):
    return ((a['w'] - b['w']).norm() / a['w'].norm()).item()


def test_syncbn_ddp_matches_single_process(gpu, tmp_path):
    """Split batch (2 images per rank) vs one process on all 4.  The BN statistics are identical up to
    fp64 summation order, but a 1-ulp change of a BN scale flips bf16 roundings that the ~100-layer
    forward/backward at random init amplifies; the update is therefore compared against a measured
    noise floor: the same single-process step on a 0.4 %-perturbed input."""
    one = _run(1, tmp_path / 'one.pt', tmp_path)
    two = _run(2, tmp_path / 'two.pt', tmp_path)
    pert = _run(1, tmp_path / 'pert.pt', tmp_path, perturb=True)
    rel = [((a - b).norm() / a.norm().clamp_min(1e-12)).item() for a, b in zip(one['rms'], two['rms'])]
    print('per-layer running_mean rel diff:', ' '.join(f'{r:.1e}' for r in rel))
    # the first BN layers see bit-identical inputs; a missing exchange is ~30 % already at layer 0
    assert max(rel[:16]) < 1e-5, rel[:16]
    split, floor = _upd_rel(one, two), _upd_rel(one, pert)
    print('update rel diff: split', split, 'noise floor', floor, 'loss', one['loss'], two['loss'], pert['loss'])
    assert split < 2.0 * floor + 0.05, (split, floor)
    assert abs(one['loss'] - two['loss']) < 1e-2 * abs(one['loss']), (one['loss'], two['loss'])
    # level-synchronous SyncBN exchanges: one collective per dependency level and direction instead of
    # one per BN and direction (reference SyncBatchNorm: 2 per BN)
    print('SyncBN collectives per step:', two['exchanges'], 'for', two['n_bn'], 'BNs')
    assert one['exchanges'] == 0
    assert 0 < two['exchanges'] <= 0.5 * 2 * two['n_bn'], (two['exchanges'], two['n_bn'])


def test_bench_ddp_path_two_ranks(gpu, tmp_path):
    """The driver's multi-GPU bench invocation (torch.distributed.run, one rank per device) rehearsed
    with 2 ranks on this one GPU over gloo: DDP bucketing + SyncBN + GPU augmentation feed + the JSON
    contract (whole-job images/sec, n_gpus, dp2)."""
    import json
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, BENCH_DIST_BACKEND='gloo', BENCH_SAME_DEVICE='1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3',
           '--warmup', '2', '--batch', '2', '--size', '64', '--train-images', '8', '--val-images', '4', '--full']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(line) == 1, r.stdout   # rank 0 prints exactly one JSON line
    d = json.loads(line[0])
    assert d['n_gpus'] == 2 and d['config']['parallelism'] == 'dp2' and d['config']['global_batch'] == 4
    assert d['value'] > 0 and d['steps'] == 3 and d['warmup'] == 2 and d['config']['syncbn']
    # the multi-GPU evidence pass: bucket timings, SyncBN exchange count, knock-out step time
    c = d['comm']
    assert c['world_size'] == 2 and c['buckets'] and c['syncbn_exchanges_per_step'] > 0
    assert c['step_ms_comm_off'] > 0 and c['instrumented_step_ms'] > 0


def test_bench_rccl_path_world1(gpu, tmp_path):
    """The RCCL code path on the real backend: one rank over `nccl` (RCCL) with --ddp, so the process
    group, the bucketed gradient all-reduce of the arena (rebuilt in grad-ready order after step 1) and the
    step's RCCL calls all run on the GPU (one device -> world size 1; more ranks are the driver's 8-GPU
    runs).  --graph-ddp off: the uncaptured step, whose per-bucket RCCL evidence pass this checks."""
    import json
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--ddp',
           '--steps', '3', '--warmup', '2', '--batch', '4', '--size', '64', '--train-images', '8',
           '--val-images', '4', '--graph-ddp', 'off', '--full']
    r = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    errs = [ln for ln in r.stderr.splitlines() if 'rror' in ln or 'what()' in ln or 'Exception' in ln][:20]
    assert r.returncode == 0, '\n'.join(errs) + '\n...\n' + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(line) == 1, r.stdout
    d = json.loads(line[0])
    assert d['n_gpus'] == 1 and d['value'] > 0 and d['config']['hipgraph'] is False
    c = d['comm']   # RCCL on-stream durations of every gradient bucket (TORCH_NCCL_ENABLE_TIMING)
    assert c['world_size'] == 1 and c['rccl_version'] and c['buckets']
    assert all(b['rccl_ms'] is not None and b['rccl_ms'] >= 0 for b in c['buckets']), c['buckets']
    assert c['buckets_rebuilt_in_ready_order'], c


def test_main_torchrun_world1_graph(gpu, tmp_path):
    """``torchrun --nproc_per_node=1 main.py`` on the fused engine: world size 1 attaches no collective, so
    the step IS graph-captured (use_graph on) and the run exits cleanly (round-3 advisor: a world-1
    bucketer inside the capture aborted in the process-group watchdog)."""
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'main.py'), '--dataset', 'synthetic',
           '--synthetic_num', '16', '4', '4', '--synthetic_size', '64', '--crop_size', '64', '--total_epoch', '2',
           '--warmup_epochs', '0', '--train_bs', '4', '--val_bs', '4', '--base_workers', '0', '--model', 'ducknet',
           '--base_channel', '8', '--no_progress_bar', '--save_dir', str(tmp_path / 'save'),
           '--data_root', str(tmp_path / 'data'), '--graph_warmup', '1']
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / 'save' / 'medseg_trainer.log').read()   # MyConfig.logger_name
    assert 'hipGraph capture on' in log and 'gradient bucketer off' in log, log[-2000:]
    assert os.path.isfile(tmp_path / 'save' / 'last.pth')


def test_graph_captured_rccl_step_bitwise_world1(gpu, tmp_path):
    """The multi-rank step captured in ONE hipGraph with its RCCL calls (gradient bucket all-reduces, the
    bucketer attached at world 1) replays bitwise like the eager multi-rank step: parameters and every
    step's loss (tools/graph_ddp_check.py under torchrun, the real `nccl` backend)."""
    import json
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'tools', 'graph_ddp_check.py')]
    r = subprocess.run(cmd, env=dict(os.environ, GDC_STEPS='5'), capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert r.returncode == 0 and len(line) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads(line[0])
    assert d['graph_captured'] and d['bucketer'] and d['buckets'] >= 1 and d['buckets_rebuilt'], d
    assert all(d['losses_equal']) and d['n_mismatch'] == 0, d


def test_bench_rccl_graph_world1(gpu, tmp_path):
    """bench.py's multi-rank mode with --graph-ddp on: the RCCL step is hipGraph-captured and benches."""
    import json
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--ddp',
           '--steps', '3', '--warmup', '2', '--batch', '4', '--size', '64', '--train-images', '8',
           '--val-images', '4', '--graph-ddp', 'on']
    r = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    d = json.loads(line[0])
    assert d['config']['hipgraph'] is True and d['value'] > 0 and d['n_gpus'] == 1
