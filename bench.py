"""Headline benchmark: env-steps/s of the batched MI355X physics step.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Both forms work for N > 1: without RANK in the environment the script is its
own launcher (`launch_ranks`: N fresh child processes, one per GPU, started
before this process has imported torch or touched the GPU -- the stand-in for
the reference's one-process-per-env fan-out, scripts/vec_env.py:396-465); under
torchrun it is one of the ranks.  `--dry-run` takes the same launcher, sharding
and gather with the gloo backend and no kernels (CPU test of the N > 1 path).

A "step" is one control step of the whole batch: one launch of the fused kernel
(n_sub_steps physics steps + task observation + reward) on actions that are
already resident in HBM, including the episode resets that fall inside the
timed region (cheetah: 200 settle steps per reset).  Workload at N=1 is the
configuration BASELINE.json's metric is quoted on: cheetah-run, batch 8192,
fp32.

N>1 (one process per GPU, `dm_control_amd.distributed`): envs are independent,
so the env axis is sharded contiguously and NO collective runs in the step.
  default          weak scaling: --batch envs per GPU (8192); `value` is this.
                   For N > 1 with --full the same line also carries `strong`:
                   BASELINE configs[3], humanoid-walk with 8192 envs in total
                   sharded shard_range(8192, N, rank) per GPU (1024 per GPU at
                   N = 8)
  --global-batch G strong scaling only: G envs in total of --domain/--task
The only collective is the RCCL all-gather of per-env episode returns on the
reporting path, after the timed region.

Rank 0 prints ONE JSON line with `roofline` (HIP events on the batch's own
stream).  A plain run does only that: set-up, warm-up, the timed steps, the
line.  `--full` adds the legs that take runs of their own: at N=1
`cpu_baseline` (the fp64 CPU oracle = "port"; libmujoco itself is a closed
binary that is not available here) including the second half of BASELINE's
metric, qpos rel-err vs the CPU step (teacher-forced per step, and
free-running at 100 / 1000 steps with the step of the first contact-count
mismatch), and `tolerance_compliant` (a short fp64 leg); at N>1 `strong`.

`--dump-outputs DIR` writes what the last timed step computed, as a caller of
the step receives it, to DIR/<name>.npy (`qpos`, `qvel`, and `observation`,
`reward` where the kernel computes the task; [env][k], the batch's precision;
a fixed sample of envs when the whole batch exceeds DUMP_BYTES).  The actions
and initial states are seeded, so two builds can be compared output for output.
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

_ROOT = os.path.dirname(os.path.abspath(__file__))
if _ROOT not in sys.path:
  sys.path.insert(0, _ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md, chip-level parameters
SIMDS = 1024            # 256 CUs x 4
VALU_CYCLES = 2         # wave64 fp32 VALU instruction on a SIMD-32: peak issue rate
VALU_CYCLES_ONE_WAVE = 4  # what a wave that has the SIMD to itself sustains
CLOCK_GHZ = 2.4
DUMP_BYTES = 60*10**6   # --dump-outputs: at most this much array data in all


def algorithmic_bytes_per_env_step(info, real_size):
  """state in, state + observation + reward out."""
  reads = info.nq + info.nv + info.nu + info.nv          # qpos qvel ctrl warm
  writes = info.nq + info.nv + info.nv + info.nobs + 1   # + obs + reward
  return (reads + writes)*real_size


def counters_for(code_object, batch):
  """PMC figures of THIS code object at THIS batch size, or None.

  rocprofv3 counters cannot be collected from inside the timed run; they come
  from separate `--pmc` passes of this same script (profiles/README.md,
  tools/collect_counters.py).  Each summary records the code object it was
  measured on (the content hash in the .hsaco file name: model, precision,
  kernel sources and flags), so a changed kernel never inherits old numbers.
  """
  tag = os.path.basename(code_object).replace('dmc_', '').replace('.hsaco', '')
  path = os.path.join(_ROOT, 'profiles', 'counters_%s_b%d.json' % (tag, batch))
  try:
    with open(path) as f:
      return json.load(f)
  except (OSError, ValueError):
    return None


def usable_cores():
  """Host cores this process may actually use (affinity and cgroup quota)."""
  n = os.cpu_count() or 1
  try:
    n = min(n, len(os.sched_getaffinity(0)))
  except AttributeError:
    pass
  try:
    with open('/sys/fs/cgroup/cpu.max') as f:
      quota, period = f.read().split()
    if quota != 'max':
      n = min(n, max(1, int(float(quota)/float(period))))
  except (OSError, ValueError):
    pass
  return n


def _compiled_model(domain):
  from dm_control_amd import suite as _suite  # host logic only (model compile)
  from dm_control_amd.mjcf import compiler
  xml, assets = getattr(_suite, domain).get_model_and_assets()
  return compiler.from_xml_string(xml, assets)


def load_env(domain, task, seed, environment_kwargs):
  """`suite.load`, or -- `--domain soccer --task 2v2` -- BASELINE configs[4]:
  `locomotion.soccer.load(team_size)` with humanoid walkers."""
  if domain == 'soccer':
    from dm_control_amd.locomotion import soccer
    return soccer.load(int(task.split('v')[0]), random_state=seed,
                       environment_kwargs=environment_kwargs)
  from dm_control_amd import suite
  return suite.load(domain, task, task_kwargs={'random': seed},
                    environment_kwargs=environment_kwargs)


def cpu_baseline(domain, task, nsub, budget_s=12.0, gpu_batch=None,
                 free_run_steps=1000, gpu_batch_model=None):
  """Times the fp64 oracle (OpenMP over envs) on a bounded sample.

  With `gpu_batch` (the benchmarked batch) the same leg also reports the
  second half of BASELINE's metric, "qpos rel-err vs CPU mj_step".
  """
  from oracle import oracle
  model = gpu_batch_model if gpu_batch_model is not None else _compiled_model(domain)
  # rebuild the oracle natively for this host (the in-tree .so is generic x86-64)
  lib = None
  try:
    out = os.path.join('/tmp', 'libmjoracle_native_%d.so' % os.getpid())
    oracle.build(force=True, cflags=['-O3', '-march=native', '-fopenmp', '-fPIC',
                                     '-std=c99', '-ffp-contract=off'], out=out)
    lib = oracle.load(out)
  except Exception:  # pylint: disable=broad-except
    lib = oracle.load()
  om = oracle.OracleModel(model, lib)
  _progress('cpu baseline: oracle loaded')
  cores = usable_cores()
  nenv = (64 if model.nv < 100 else 2)*cores      # a 2v2 pitch is ~13 ms per physics step
  datas = [oracle.OracleData(om) for _ in range(nenv)]
  rs = np.random.RandomState(0)
  lim = model.jnt_limited.astype(bool)
  for d in datas:
    if domain == 'cheetah':
      lo, hi = model.jnt_range[lim].T
      d.qpos[lim] = rs.uniform(lo, hi)
    d.step1()
  ctrl = rs.uniform(-1, 1, (nenv, model.nu))
  used = oracle.batch_step(om, datas, ctrl, nsub, cores)      # warm-up
  t0 = time.time()
  oracle.batch_step(om, datas, ctrl, nsub, cores)
  probe = max(time.time() - t0, 1e-4)
  reps = int(max(5, min(20000, budget_s/probe)))
  t0 = time.time()
  for r in range(reps):
    if r % 16 == 0:
      ctrl = rs.uniform(-1, 1, (nenv, model.nu))
    oracle.batch_step(om, datas, ctrl, nsub, cores)
  dt = time.time() - t0
  out = {
      'value': nenv*reps/dt, 'unit': 'env-steps/s', 'cores': int(used),
      'kind': 'port',
      'sample': '%s-%s: %d envs x %d control steps (%d physics steps each), '
                'fp64 C restatement of mj_step, OpenMP over envs, %.1f s'
                % (domain, task, nenv, reps, nsub, dt)}
  _progress('cpu baseline timed: %.3g env-steps/s' % out['value'])
  if gpu_batch is not None:
    out['qpos_rel_err'] = {
        'definition': 'max|q_gpu - q_cpu| / max(1, max|q_cpu|) per env; CPU = '
                      'fp64 oracle (KAT-pinned restatement, not libmujoco)',
        'teacher_forced': _rel_err_sample(gpu_batch, om, oracle, nsub,
                                          nenv=64 if model.nv < 100 else 8,
                                          steps=20 if model.nv < 100 else 4),
        'free_run': _free_run_sample(gpu_batch, om, oracle, nsub, cores,
                                     nenv=64 if model.nv < 100 else 8,
                                     steps=free_run_steps)}
  return out


def _start_states(gpu_batch, nenv):
  from dm_control_amd import wrapper as W
  q0 = gpu_batch.read(W.FIELD_QPOS).T[:nenv].astype(np.float64)
  v0 = gpu_batch.read(W.FIELD_QVEL).T[:nenv].astype(np.float64)
  w0 = gpu_batch.read(W.FIELD_WARMSTART).T[:nenv].astype(np.float64)
  return q0, v0, w0


def _twin_batch(gpu_batch, nenv):
  """A small batch on the same code object as the bench, same task data."""
  from dm_control_amd import wrapper as W
  hb = W.HipBatch(gpu_batch.model, nenv)
  if gpu_batch.model.info.ntaskdata:
    hb.write(W.FIELD_TASKDATA, gpu_batch.read(W.FIELD_TASKDATA)[:, :nenv])
  return hb


def _rel(q, ref):
  return np.abs(q - ref).max(axis=1)/np.maximum(1, np.abs(ref).max(axis=1))


def _rel_err_sample(gpu_batch, om, oracle, nsub, nenv=64, steps=20):
  """Teacher-forced: both sides restart every control step from the oracle's
  state (incl. its warm start) under the same controls."""
  from dm_control_amd import wrapper as W
  model = om.model
  q0, v0, _ = _start_states(gpu_batch, nenv)
  nenv = len(q0)
  hb = _twin_batch(gpu_batch, nenv)
  datas = [oracle.OracleData(om) for _ in range(nenv)]
  for i, d in enumerate(datas):
    d.qpos[:] = q0[i]
    d.qvel[:] = v0[i]
    d.step1()
  rs = np.random.RandomState(1)
  errs = []
  for _ in range(steps):
    oq = np.array([d.qpos.copy() for d in datas])
    ov = np.array([d.qvel.copy() for d in datas])
    ow = np.array([d.qacc_warmstart.copy() for d in datas])
    hb.set_state(oq.T, ov.T, ow.T)
    ctrl = rs.uniform(-1, 1, (nenv, model.nu))
    hb.step_host(ctrl, nsub)
    q = hb.read(W.FIELD_QPOS).T.astype(np.float64)
    for i, d in enumerate(datas):
      d.ctrl[:] = ctrl[i]
      for _ in range(nsub):
        d.physics_step()
    nq = np.array([d.qpos.copy() for d in datas])
    errs.append(_rel(q, nq))
  hb.free()
  e = np.concatenate(errs)
  return {'median': float(np.median(e)), 'p99': float(np.percentile(e, 99)),
          'max': float(e.max()),
          'sample': '%d envs from the benchmarked batch x %d control steps, same '
                    'code object, U(-1,1) controls' % (nenv, steps)}


def _free_run_sample(gpu_batch, om, oracle, nsub, cores, nenv=64, steps=1000):
  """Free-running: both sides start from the same states of the benchmarked
  batch and see the same U(-1,1) controls for `steps` control steps; no state
  is ever copied across.  Reports the error at 100 and `steps` steps, the share
  of envs within BASELINE's 1e-4, the horizon (control steps an env stays within
  1e-4 of the oracle) and the control step at which an env's contact count
  first differs from the oracle's (from there on the two are different
  trajectories of a chaotic system, in any pair of implementations)."""
  from dm_control_amd import wrapper as W
  model = om.model
  q0, v0, w0 = _start_states(gpu_batch, nenv)
  nenv = len(q0)
  hb = _twin_batch(gpu_batch, nenv)
  hb.set_state(q0.T, v0.T, w0.T)
  datas = [oracle.OracleData(om) for _ in range(nenv)]
  for i, d in enumerate(datas):
    d.qpos[:] = q0[i]
    d.qvel[:] = v0[i]
    d.qacc_warmstart[:] = w0[i]
    d.step1()
  rs = np.random.RandomState(2)
  first = np.full(nenv, steps + 1)
  horizon = np.full(nenv, steps)          # steps completed within 1e-4
  alive = np.ones(nenv, bool)
  marks = {}
  for t in range(steps):
    ctrl = rs.uniform(-1, 1, (nenv, model.nu))
    hb.step_host(ctrl, nsub)
    # contacts the LAST physics step of this control step acted on
    if nsub > 1:
      oracle.batch_step(om, datas, ctrl, nsub - 1, cores)
    ref = np.array([d.ncon for d in datas])
    oracle.batch_step(om, datas, ctrl, 1, cores)
    ncon = hb.read(W.FIELD_STATS)[0]
    new = (ncon != ref) & (first > steps)
    first[new] = t + 1
    q = hb.read(W.FIELD_QPOS).T.astype(np.float64)
    e = _rel(q, np.array([d.qpos.copy() for d in datas]))
    left = alive & ~(e <= 1e-4)           # NaN counts as having left
    horizon[left] = t
    alive &= ~left
    if t + 1 in (100, steps) or (steps < 100 and t + 1 == steps//2):
      marks['step_%d' % (t + 1)] = {
          'median': float(np.median(e)), 'p90': float(np.percentile(e, 90)),
          'max': float(e.max()), 'frac_within_1e-4': float(np.mean(e <= 1e-4))}
  hb.free()
  out = dict(marks)
  out['horizon_steps_within_1e-4'] = {
      'min': int(horizon.min()), 'median': float(np.median(horizon)),
      'envs_within_for_all_%d_steps' % steps: int(alive.sum()), 'envs': int(nenv)}
  mism = first <= steps
  out['first_contact_count_mismatch'] = {
      'envs': int(mism.sum()),
      'earliest_step': int(first.min()) if mism.any() else None}
  out['sample'] = ('%d envs from the benchmarked batch, %d free-running control '
                   'steps, same code object, U(-1,1) controls' % (nenv, steps))
  return out


def dump_outputs(batch, directory, prefix=''):
  """Writes the step's outputs of every env (or of a seeded sample of envs,
  the same for the same batch size) as float32 / float64 .npy files."""
  from dm_control_amd import wrapper as W
  info = batch.model.info
  fields = [('qpos', W.FIELD_QPOS), ('qvel', W.FIELD_QVEL)]
  if info.nobs > 0:
    fields += [('observation', W.FIELD_OBS), ('reward', W.FIELD_REWARD)]
  arrays = {}
  for name, field in fields:
    a = batch.read(field)
    arrays[name] = a if field in (W.FIELD_OBS, W.FIELD_REWARD) else a.T
  nenv = batch.nenv
  per_env = sum(a.nbytes for a in arrays.values())//nenv
  keep = None
  if per_env*nenv > DUMP_BYTES:
    keep = np.sort(np.random.RandomState(0).choice(
        nenv, DUMP_BYTES//per_env, replace=False))
  os.makedirs(directory, exist_ok=True)
  for name, a in arrays.items():
    if keep is not None:
      a = a[keep]
    np.save(os.path.join(directory, prefix + name + '.npy'), np.ascontiguousarray(a))
  sys.stderr.write('bench: outputs of the last timed step -> %s (%s envs)\n'
                   % (directory, nenv if keep is None else '%d of %d' % (len(keep), nenv)))


def _progress(msg):
  """$DMC_BENCH_PROGRESS=1: stage markers on stderr (long legs: soccer)."""
  if os.environ.get('DMC_BENCH_PROGRESS'):
    sys.stderr.write('[bench %.1fs] %s\n' % (time.time() - _T0, msg))
    sys.stderr.flush()


_T0 = time.time()


def _positive(text):
  n = int(text)
  if n < 1:
    raise argparse.ArgumentTypeError('must be at least 1')
  return n


def parse_args(argv=None):
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpus', type=int, default=1)
  ap.add_argument('--steps', type=_positive, default=1000,
                  help='timed control steps')
  ap.add_argument('--warmup', type=int, default=50)
  ap.add_argument('--domain', default='cheetah')
  ap.add_argument('--task', default='run')
  ap.add_argument('--batch', type=int, default=8192,
                  help='envs per GPU (weak scaling)')
  ap.add_argument('--global-batch', type=int, default=None,
                  help='total envs, sharded over the GPUs (strong scaling only)')
  ap.add_argument('--precision', default='f32', choices=['f32', 'f64', 'mixed'],
                  help='mixed: fp32 arithmetic, qpos/qvel carried as fp64 (hi, lo) pairs')
  ap.add_argument('--full', action='store_true',
                  help='also the CPU-oracle baseline and its error samples and the '
                       'fp64 (tolerance-compliant) leg at N = 1, the humanoid-walk '
                       'strong-scaling leg at N > 1')
  ap.add_argument('--no-cpu-baseline', action='store_true',
                  help='with --full: skip the CPU-oracle baseline and the fp64 leg')
  ap.add_argument('--no-compliant-leg', action='store_true',
                  help='with --full: skip the short fp64 (tolerance-compliant) leg at N = 1')
  ap.add_argument('--no-strong-leg', action='store_true',
                  help='with --full: skip the humanoid-walk strong-scaling leg at N > 1')
  ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                  help='write the outputs of the last timed step to DIR/<name>.npy')
  ap.add_argument('--dry-run', action='store_true',
                  help='launcher, sharding and gather only (gloo, no kernels)')
  return ap.parse_args(argv)


# -- N > 1 without torchrun: this script starts its own ranks --------------------

def _free_port():
  import socket
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    return s.getsockname()[1]


def launch_ranks(ngpus, argv):
  """Starts one fresh process per GPU and relays rank 0's JSON line.

  Runs in a parent that has NOT imported torch or made any HIP call (children
  are new interpreters: `subprocess`, never an exec of a process that touched
  the GPU).  Every child gets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* like a
  torchrun worker.  Returns the exit code: non-zero if any rank failed (the
  remaining ranks are then terminated, so a dead rank cannot leave the others
  hanging in a collective).
  """
  import subprocess
  env = dict(os.environ)
  env.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()),
             WORLD_SIZE=str(ngpus), LOCAL_WORLD_SIZE=str(ngpus))
  env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  env.setdefault('OMP_NUM_THREADS', '1')
  procs = []
  for rank in range(ngpus):
    e = dict(env, RANK=str(rank), LOCAL_RANK=str(rank))
    procs.append(subprocess.Popen(
        [sys.executable, os.path.abspath(__file__)] + list(argv), env=e,
        stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL))
  out, _ = procs[0].communicate()
  rc = procs[0].returncode
  deadline = time.time() + 120
  for p in procs[1:]:
    if rc != 0:
      p.terminate()
    try:
      p.wait(timeout=max(1, deadline - time.time()))
    except subprocess.TimeoutExpired:
      p.kill()
      p.wait()
    rc = rc or p.returncode
  # rank 0's stdout carries the JSON line; anything else a library printed there
  # (gloo's connection banner) goes to stderr so that stdout stays one line
  for text in out.decode().splitlines():
    (sys.stdout if text.startswith('{') else sys.stderr).write(text + '\n')
  sys.stdout.flush()
  return rc


def shard_of(args, world, rank, global_batch=None):
  """(scaling, total envs, [start, stop), per-env seeds) of this rank."""
  from dm_control_amd import distributed
  if global_batch is None:
    global_batch = args.global_batch
  if global_batch is not None:
    scaling, total = 'strong', int(global_batch)
    start, stop = distributed.shard_range(total, world, rank)
  else:
    scaling, total = 'weak', args.batch*world
    start, stop = rank*args.batch, (rank + 1)*args.batch
    assert (start, stop) == distributed.shard_range(total, world, rank)
  seeds = distributed.env_seeds(1000, total, world, rank)
  assert len(seeds) == stop - start
  return scaling, total, (start, stop), seeds


def dry_run(args):
  """The N > 1 plumbing without a GPU: process group (gloo), shards, per-env
  seeds, the reporting all-gather, rank 0's line."""
  import torch
  import torch.distributed as dist
  from dm_control_amd import distributed
  rank, world = distributed.init_process_group(
      'gloo', single_rank_group='RANK' in os.environ)
  if world != args.gpus:
    raise SystemExit('--gpus %d but the launcher started %d rank(s)'
                     % (args.gpus, world))
  scaling, total, (start, stop), seeds = shard_of(args, world, rank)
  # each rank "simulates" its shard: the return of env i depends on its global
  # seed only, so the gathered vector must not depend on the sharding
  local = torch.from_numpy((seeds - 1000).astype(np.float32))*0.5 + 1.0
  full = distributed.gather_episode_returns(local, total)
  ok = bool(torch.equal(full, torch.arange(total, dtype=torch.float32)*0.5 + 1.0))
  in_group = dist.is_available() and dist.is_initialized()
  if rank == 0:
    print(json.dumps({
        'metric': 'env-steps/sec', 'value': None, 'unit': 'env-steps/s',
        'dry_run': True, 'n_gpus': args.gpus, 'scaling': scaling,
        'world_size_seen': dist.get_world_size() if in_group else 1,
        'backend': dist.get_backend() if in_group else None,
        'global_batch': total, 'rank0_shard': [start, stop],
        'gathered_returns': int(full.numel()), 'gather_ok': ok}))
  if in_group:
    dist.barrier()
    dist.destroy_process_group()
  return 0 if ok else 1


# -- one timed leg ---------------------------------------------------------------

def measure(domain, task, precision, seeds, local_rank, steps, warmup, in_group):
  """Warm-up, then `steps` timed control steps of `len(seeds)` envs on this
  rank's GPU, bracketed by barrier + synchronize; elapsed = MAX over ranks.
  Returns (figures, env): the caller frees or reuses the env."""
  import torch
  import torch.distributed as dist
  nlocal = len(seeds)
  env = load_env(domain, task, int(seeds[0]),
                 {'batch_size': nlocal, 'device': local_rank,
                  'precision': precision, 'device_init': True})
  physics, task_obj = env.physics, env.task
  batch = physics.batch
  info = batch.model.info
  nsub = env._n_sub_steps                      # pylint: disable=protected-access
  step_limit = env._step_limit                 # pylint: disable=protected-access
  tdtype = torch.float64 if precision == 'f64' else torch.float32
  dev = torch.device('cuda', local_rank)
  gen = torch.Generator(device=dev)
  gen.manual_seed(int(seeds[0]))
  # 16 steps of actions U(-1,1), resident in HBM, [t][env][nu]
  pool = torch.rand(16, nlocal, info.nu, device=dev, dtype=tdtype,
                    generator=gen)*2 - 1
  torch.cuda.synchronize(dev)

  state = {'count': 0, 'ev_ms': 0.0, 'ev_launches': 0, 'timing': False,
           'resets': 0}

  def reset_episode(timed=False):
    with physics.reset_context():
      task_obj.initialize_episode(physics)
    state['count'] = 0
    state['resets'] += int(timed)

  def run(nsteps, timed):
    # One launch per control step; the launches of up to 16 steps are issued by
    # one C call (dmc_batch_step_n) so that the small models are not bound by
    # the interpreter's per-step overhead.
    done = 0
    while done < nsteps:
      if state['count'] >= step_limit:
        if timed and state['timing']:
          ms, n = batch.timer_stop()
          state['ev_ms'] += ms; state['ev_launches'] += n
          state['timing'] = False
        reset_episode(timed)
      if timed and not state['timing']:
        batch.timer_start()
        state['timing'] = True
      chunk = int(min(16, nsteps - done, step_limit - state['count']))
      batch.step_device_n(pool.data_ptr(), 1, info.nu, nlocal*info.nu,
                          chunk, nsub)
      state['count'] += chunk
      done += chunk
    if timed and state['timing']:
      ms, n = batch.timer_stop()
      state['ev_ms'] += ms; state['ev_launches'] += n
      state['timing'] = False

  _progress('env built (%s), first reset' % physics.kernel_shape)
  reset_episode()
  _progress('warm-up')
  run(warmup, False)
  batch.sync()
  _progress('timed region')
  torch.cuda.synchronize(dev)
  if in_group:
    dist.barrier()
  t0 = time.perf_counter()
  run(steps, True)
  batch.sync()
  torch.cuda.synchronize(dev)
  elapsed = time.perf_counter() - t0
  if in_group:
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    dist.barrier()
  return {'elapsed': elapsed, 'nsub': nsub, 'resets': state['resets'],
          'kernel_ms': state['ev_ms']/max(1, state['ev_launches']),
          'nlocal': nlocal}, env


def main(argv=None):
  argv = sys.argv[1:] if argv is None else list(argv)
  args = parse_args(argv)
  if args.gpus > 1 and 'RANK' not in os.environ:
    # plain `python bench.py --gpus N`: be the launcher (nothing GPU-related has
    # been imported yet in this process)
    return launch_ranks(args.gpus, argv)
  if args.dry_run:
    return dry_run(args)

  import torch
  import torch.distributed as dist
  from dm_control_amd import distributed, wrapper
  # under a launcher (RANK set) the RCCL path is taken even for one rank, so the
  # process-group / all-gather code is exercised on a single-GPU box as well
  rank, world = distributed.init_process_group(
      'nccl', single_rank_group='RANK' in os.environ)
  if world != args.gpus:
    raise SystemExit('--gpus %d but the launcher started %d rank(s)'
                     % (args.gpus, world))
  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  in_group = dist.is_available() and dist.is_initialized()
  dev = torch.device('cuda', local_rank)

  scaling, total_envs, _, seeds = shard_of(args, world, rank)
  fig, env = measure(args.domain, args.task, args.precision, seeds, local_rank,
                     args.steps, args.warmup, in_group)
  physics = env.physics
  batch = physics.batch
  info = batch.model.info
  nlocal, nsub, elapsed = fig['nlocal'], fig['nsub'], fig['elapsed']

  _progress('timed region done: %.3f s' % elapsed)
  # reporting path: all-gather of per-env episode returns over RCCL/xGMI
  returns = torch.from_numpy(
      batch.read(wrapper.FIELD_RETURN).astype(np.float32)).to(dev)
  returns = distributed.gather_episode_returns(returns, total_envs)
  warn = batch.read(wrapper.FIELD_WARN)
  if args.dump_outputs:
    dump_outputs(batch, args.dump_outputs, '' if world == 1 else 'rank%d_' % rank)

  line = None
  if rank == 0:
    value = total_envs*args.steps/elapsed
    kernel_ms = fig['kernel_ms']
    bytes_per_launch = algorithmic_bytes_per_env_step(
        info, info.real_size)*nlocal
    achieved = bytes_per_launch/(kernel_ms*1e-3)/1e9 if kernel_ms > 0 else 0.0
    code_object = physics.code_object
    counters = counters_for(code_object, nlocal) or {}
    valu = None
    if counters.get('valu_insts_per_launch') and kernel_ms > 0:
      insts = counters['valu_insts_per_launch']
      simd_cycles = SIMDS*kernel_ms*1e-3*CLOCK_GHZ*1e9
      valu = {
          'insts_per_wave': insts/max(1, counters.get('waves_per_launch', 1)),
          'valu_busy_on_occupied_simd': counters.get('valu_busy'),
          # against the SIMD's peak issue rate (one wave64 fp32 op per 2 cycles)
          'chip_issue_frac': insts*VALU_CYCLES/simd_cycles,
          # against what one wave per SIMD can sustain (4 cycles per op)
          'chip_issue_frac_at_one_wave_per_simd':
              insts*VALU_CYCLES_ONE_WAVE/simd_cycles,
          'source': counters.get('source')}
    resets = ', %d episode reset(s) inside the timed region' % fig['resets'] \
        if fig['resets'] else ''
    line = {
        'metric': 'env-steps/sec', 'value': value, 'unit': 'env-steps/s',
        'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': elapsed/args.steps*1e3, 'higher_is_better': True,
        'scaling': scaling, 'vs_baseline': None,
        'dtype': {'mixed': 'f32 (state carried in f64)'}.get(args.precision, args.precision),
        'data': 'synthetic',
        'config': {
            'workload': '%s-%s, %d envs per GPU (dm_control.suite, %d physics '
                        'substeps per env-step%s)'
                        % (args.domain, args.task, nlocal, nsub, resets),
            'global_batch': total_envs,
            'parallelism': 'env-shard x%d (%s: %s)' % (
                world, scaling,
                '%d envs in total' % total_envs if scaling == 'strong'
                else '%d envs per GPU' % args.batch),
            'world_size_seen': dist.get_world_size() if in_group else 1,
            'collective_backend': dist.get_backend() if in_group else None,
            'actions': 'U(-1,1), device-resident',
            'code_object': os.path.basename(code_object),
            'kernel_shape': physics.kernel_shape},
        'roofline': {
            # the contract's figure (north_star: achieved HBM GB/s vs 8 TB/s);
            # what actually limits the kernel is VALU issue, see `valu`
            'bound': 'hbm',
            'limited_by': ('dependent-memory-latency (one wavefront per env: tiles and tables '
                           'travel through HBM / LDS on a serial chain)'
                           if 'team mode' in physics.kernel_shape else 'valu-issue'),
            'achieved': achieved, 'peak': HBM_PEAK_GBS,
            'unit': 'GB/s', 'frac': achieved/HBM_PEAK_GBS,
            'traffic': counters.get('traffic_bytes_per_launch'),
            'traffic_unit': 'bytes/launch (rocprofv3 FETCH_SIZE+WRITE_SIZE, '
                            'separate passes on this code object, see profiles/)',
            'valu': valu,
            'kernel': 'dmc_step',
            'kernel_ms_avg': kernel_ms,
            'algorithmic_bytes_per_launch': bytes_per_launch},
        'physics_steps_per_s': value*nsub,   # excl. the settle steps of episode resets
        'mean_episode_return': float(returns.mean().item()),
        'envs_with_warnings': int((warn != 0).sum()),
    }
    if world == 1 and args.full and not args.no_cpu_baseline:
      line['cpu_baseline'] = cpu_baseline(
          args.domain, args.task, nsub, gpu_batch=batch,
          gpu_batch_model=physics.model,
          free_run_steps=1000 if physics.model.nv < 100 else 40)
      line['tolerance'] = tolerance_verdict(
          line['dtype'], line['cpu_baseline']['qpos_rel_err']['free_run'])
  physics.free()

  # BASELINE's metric has two halves (throughput AND qpos within 1e-4 of the CPU
  # step over 1000 steps).  The fp64 build meets the second half for every env of
  # the smooth / planar-contact domains, so its figure rides in the same line.
  if (world == 1 and args.full and args.precision != 'f64'
      and not args.no_compliant_leg and not args.no_cpu_baseline):
    fsteps, fwarm = min(args.steps, 200), min(args.warmup, 20)
    if args.domain == 'soccer':
      # A second big-scratch code object in the same process inherits the first
      # one's scratch set-up on the shared hardware queue (measured: the fp64
      # pitch took 430 ms per step after the fp32 leg, 59 ms on its own,
      # tools/debug/two_legs.py): this leg runs as a child process.
      line['tolerance_compliant'] = compliant_leg_in_a_child(args, fsteps, fwarm)
      f64 = env64 = None
    else:
      f64, env64 = measure(args.domain, args.task, 'f64', seeds, local_rank,
                           fsteps, fwarm, in_group)
    if rank == 0 and env64 is not None:
      b64 = env64.physics.batch
      i64 = b64.model.info
      fr = cpu_baseline(args.domain, args.task, f64['nsub'], budget_s=1.0,
                        gpu_batch=b64, gpu_batch_model=env64.physics.model,
                        free_run_steps=1000 if env64.physics.model.nv < 100 else 40)['qpos_rel_err']
      bytes64 = algorithmic_bytes_per_env_step(i64, i64.real_size)*f64['nlocal']
      line['tolerance_compliant'] = {
          'dtype': 'f64', 'value': total_envs*fsteps/f64['elapsed'],
          'unit': 'env-steps/s', 'steps': fsteps, 'warmup': fwarm,
          'ms_per_step': f64['elapsed']/fsteps*1e3,
          'kernel_ms_avg': f64['kernel_ms'],
          'roofline_frac': bytes64/(f64['kernel_ms']*1e-3)/1e9/HBM_PEAK_GBS
                           if f64['kernel_ms'] > 0 else None,
          'code_object': os.path.basename(env64.physics.code_object),
          'kernel_shape': env64.physics.kernel_shape,
          'qpos_rel_err': fr,
          'tolerance': tolerance_verdict('f64', fr['free_run'])}
    if env64 is not None:
      env64.physics.free()

  # N > 1: BASELINE configs[3] in the same line (strong scaling: 8192 humanoids
  # in total, 1024 per GPU at N = 8)
  if (world > 1 and args.full and args.global_batch is None
      and not args.no_strong_leg):
    _, stotal, _, sseeds = shard_of(args, world, rank, global_batch=8192)
    ssteps, swarm = min(args.steps, 200), min(args.warmup, 20)
    sf, senv = measure('humanoid', 'walk', args.precision, sseeds, local_rank,
                       ssteps, swarm, in_group)
    sret = torch.from_numpy(senv.physics.batch.read(
        wrapper.FIELD_RETURN).astype(np.float32)).to(dev)
    sret = distributed.gather_episode_returns(sret, stotal)
    if rank == 0:
      line['strong'] = {
          'workload': 'humanoid-walk, %d envs in total = %d on rank 0 '
                      '(BASELINE configs[3]; %d physics substeps per env-step)'
                      % (stotal, sf['nlocal'], sf['nsub']),
          'scaling': 'strong', 'value': stotal*ssteps/sf['elapsed'],
          'unit': 'env-steps/s', 'steps': ssteps, 'warmup': swarm,
          'ms_per_step': sf['elapsed']/ssteps*1e3,
          'kernel_ms_avg_rank0': sf['kernel_ms'],
          'kernel_shape': senv.physics.kernel_shape,
          'gathered_returns': int(sret.numel())}
    senv.physics.free()

  if rank == 0:
    print(json.dumps(line))
  if in_group:
    dist.barrier()
    dist.destroy_process_group()
  return 0


def _child_env():
  env = dict(os.environ)
  for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
    env.pop(k, None)            # the child is a plain one-GPU run
  return env


def compliant_leg_in_a_child(args, steps, warmup):
  """The fp64 leg as `python bench.py --precision f64 ...` in a child process
  (started, not exec'ed: this process has initialised the GPU); returns the
  `tolerance_compliant` object built from the child's line."""
  cmd = [sys.executable, os.path.abspath(__file__), '--domain', args.domain, '--task', args.task,
         '--batch', str(args.batch), '--precision', 'f64', '--steps', str(steps),
         '--warmup', str(warmup), '--full', '--no-compliant-leg']
  proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        universal_newlines=True, env=_child_env())
  lines = [l for l in proc.stdout.splitlines() if l.startswith('{')]
  if proc.returncode != 0 or not lines:
    return {'dtype': 'f64', 'error': 'child leg failed (rc %d): %s'
                                     % (proc.returncode, proc.stderr[-300:])}
  c = json.loads(lines[-1])
  return {'dtype': 'f64', 'value': c['value'], 'unit': c['unit'], 'steps': c['steps'],
          'warmup': c['warmup'], 'ms_per_step': c['ms_per_step'],
          'kernel_ms_avg': c['roofline']['kernel_ms_avg'], 'roofline_frac': c['roofline']['frac'],
          'code_object': c['config']['code_object'], 'kernel_shape': c['config']['kernel_shape'],
          'qpos_rel_err': c.get('cpu_baseline', {}).get('qpos_rel_err'),
          'tolerance': c.get('tolerance'), 'process': 'child of this run'}


def tolerance_verdict(dtype, free_run):
  """Which half of BASELINE's metric this build meets, from the free-run sample."""
  last = [k for k in free_run if k.startswith('step_')]
  last = max(last, key=lambda k: int(k.split('_')[1]))
  hz = free_run['horizon_steps_within_1e-4']
  nsteps = int(last.split('_')[1])
  every = hz['envs_within_for_all_%d_steps' % nsteps] == hz['envs']
  out = {'target': 'qpos within 1e-4 rel-err of the CPU step over %d steps' % nsteps,
         'dtype': dtype, 'met_for_every_env_of_the_sample': bool(every),
         'share_of_envs': hz['envs_within_for_all_%d_steps' % nsteps]/hz['envs'],
         'horizon_steps_within_1e-4': {'min': hz['min'], 'median': hz['median']}}
  if not every and free_run['first_contact_count_mismatch']['envs']:
    out['note'] = ('envs leave the oracle\'s contact sequence (earliest step %s): '
                   'from there two implementations follow different trajectories '
                   'of a chaotic system; the horizon is the verifiable figure'
                   % free_run['first_contact_count_mismatch']['earliest_step'])
  return out


if __name__ == '__main__':
  sys.exit(main())
