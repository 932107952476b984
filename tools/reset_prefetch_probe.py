"""What the episode prefetch gives over whole episodes, and what it costs the steps.

  python tools/reset_prefetch_probe.py [--out FILE] [--batch 8192] [--episodes 4] [--ungated]

cheetah-run, fp32, device-side initialisation, bench.py's loop (chunks of 16
control steps of resident U(-1,1) actions through `step_device_n`, a reset at
the step limit).  `bench.py` times one reset, whose prefetch ran during the
warm-up; here the prefetch of every episode but the first is issued half way
through the episode before it and runs beside that episode's steps, as in
continued use.  `--reps` interleaved repetitions of each variant, medians:

  (a) `episodes` whole episodes (each: reset + 1000 control steps), wall clock
      around a device synchronisation, `Cheetah.prefetch` off / on
  (b) 128 control steps (HIP events on the batch's stream, per control step)
      alone / with a 200-substep prefetch issued right before them: the steps'
      share of the interference between the two launches

`--ungated` lifts the task's own limit on the batch size (suite/cheetah.py asks for
a prefetch up to 128 workgroups): how the limit was found, at 16384 envs.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--batch', type=int, default=8192)
  ap.add_argument('--episodes', type=int, default=4)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--ungated', action='store_true')
  args = ap.parse_args()
  import torch
  from dm_control_amd import suite
  from dm_control_amd.suite import cheetah
  if args.ungated:
    cheetah._PREFETCH_MAX_WORKGROUPS = 1 << 30   # pylint: disable=protected-access
  n = args.batch
  env = suite.load('cheetah', 'run', task_kwargs={'random': 1000},
                   environment_kwargs={'batch_size': n, 'device': 0, 'precision': 'f32',
                                       'device_init': True})
  physics, task = env.physics, env.task
  batch = physics.batch
  nu = batch.model.info.nu
  nsub = env._n_sub_steps                      # pylint: disable=protected-access
  limit = int(env._step_limit)                 # pylint: disable=protected-access
  gen = torch.Generator(device='cuda')
  gen.manual_seed(0)
  pool = torch.rand(16, n, nu, device='cuda', generator=gen)*2 - 1
  torch.cuda.synchronize()

  def reset():
    with physics.reset_context():
      task.initialize_episode(physics)

  def steps(count):
    done = 0
    while done < count:
      chunk = min(16, count - done)
      batch.step_device_n(pool.data_ptr(), 1, nu, n*nu, chunk, nsub)
      done += chunk

  def episodes(prefetch):
    task.prefetch = prefetch
    for _ in range(2):         # (the firing rule goes by the length of the episode before)
      reset()
      steps(limit)
    batch.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.episodes):
      reset()
      steps(limit)
    batch.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0)/(args.episodes*limit)*1e3

  def step_ms(beside):
    task.prefetch = False
    reset()
    steps(64)
    batch.sync()
    torch.cuda.synchronize()
    if beside:
      batch.episode_prefetch(12345, 200, stale_first=True, zero_time=True)
    batch.timer_start()
    steps(128)
    ms, count = batch.timer_stop()
    torch.cuda.synchronize()
    batch.episode_take(0, 0)   # (forget it)
    return ms/count

  out = {'workload': 'cheetah-run, %d envs, fp32, %s' % (n, physics.kernel_shape),
         'reps': args.reps, 'episodes': args.episodes, 'ungated': args.ungated}
  for name, fn, variants in (('ms_per_control_step_over_whole_episodes', episodes,
                              (('prefetch_off', False), ('prefetch_on', True))),
                             ('kernel_ms_per_control_step_128_steps', step_ms,
                              (('alone', False), ('beside_a_prefetch', True)))):
    runs = {v: [] for v, _ in variants}
    for _ in range(args.reps):
      for v, arg in variants:
        runs[v].append(fn(arg))
    out[name] = {v: {'median': float(np.median(r)), 'min': min(r), 'max': max(r)}
                 for v, r in runs.items()}
  e = out['ms_per_control_step_over_whole_episodes']
  out['env_steps_per_s'] = {v: n/(e[v]['median']*1e-3) for v in e}
  physics.free()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
