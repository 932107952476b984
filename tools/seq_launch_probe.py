"""What one launch per control step costs against one launch per sequence.

  python tools/seq_launch_probe.py [--out FILE] [--batch 8192] [--steps 16]

cheetah-run, fp32, the one-env-per-lane kernel, from the states reached after
100 control steps under U(-1,1) actions.  Every variant starts from that same
saved state, holds one action per env for the whole sequence (so that all
variants integrate the same trajectory) and is timed with the batch's HIP-event
timer; the median of `--reps` interleaved repetitions is reported:

  (a) `steps` launches of dmc_batch_step, nsub=1, outputs on
  (b) one launch with nsub=`steps`, outputs on (one observation stage in all)
  (c) as (a) with DMC_FLAG_NO_OUTPUT
  (d) dmc_batch_step_n over the same `steps` steps (one launch per chunk where
      the code object supports sequence launches, else the loop of (a))

(a)/steps against (b)/steps bounds what a sequence launch can save (the tail of
the slowest wave per launch, state round trips, launch ramp and drain, the
observation stage); (a) - (c) bounds the observation stage alone.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--batch', type=int, default=8192)
  ap.add_argument('--steps', type=int, default=16)
  ap.add_argument('--reps', type=int, default=9)
  args = ap.parse_args()
  import torch
  from dm_control_amd import suite
  from dm_control_amd import wrapper as W
  n, k = args.batch, args.steps
  env = suite.load('cheetah', 'run', task_kwargs={'random': 1000},
                   environment_kwargs={'batch_size': n, 'device': 0, 'precision': 'f32',
                                       'device_init': True})
  physics = env.physics
  batch = physics.batch
  nu = batch.model.info.nu
  with physics.reset_context():
    env.task.initialize_episode(physics)
  gen = torch.Generator(device='cuda')
  gen.manual_seed(0)
  acts = torch.rand(101, n, nu, device='cuda', generator=gen)*2 - 1
  torch.cuda.synchronize()
  batch.step_device_n(acts.data_ptr(), 1, nu, n*nu, 100, 1)
  batch.sync()
  state = [batch.read(f) for f in (W.FIELD_QPOS, W.FIELD_QVEL, W.FIELD_WARMSTART, W.FIELD_TIME)]
  held = acts[100].data_ptr()

  def a_():
    for _ in range(k):
      batch.step_device(held, 1, nu, 1, True)

  def b_():
    batch.step_device(held, 1, nu, k, True)

  def c_():
    for _ in range(k):
      batch.step_device(held, 1, nu, 1, False)

  def d_():
    batch.step_device_n(held, 1, nu, 0, k, 1, True)

  variants = (('a', a_), ('b', b_), ('c', c_), ('d', d_))
  ms = {name: [] for name, _ in variants}
  final = {}
  for rep in range(args.reps + 1):      # (the first repetition warms up)
    for name, fn in variants:
      batch.set_state(*state)
      batch.sync()
      batch.timer_start()
      fn()
      t, _ = batch.timer_stop()
      if rep:
        ms[name].append(t)
      final[name] = batch.read(W.FIELD_QPOS)
  stats = batch.read(W.FIELD_STATS)
  med = {name: float(np.median(v)) for name, v in ms.items()}
  lines = [
      'cheetah-run, %d envs, fp32, %s' % (n, physics.kernel_shape),
      'code object %s, sequence launches: %s' % (
          os.path.basename(physics.code_object),
          getattr(batch.model.info, 'seq_launch', 0)),
      'start: 100 control steps of U(-1,1) actions after reset; %d steps timed, one held action; '
      'median of %d (min .. max), HIP events' % (k, args.reps),
      'contacts per env at the end: mean %.2f, max %d' % (stats[0].mean(), stats[0].max())]
  text = {'a': '%d launches, nsub=1, outputs on' % k,
          'b': 'one launch, nsub=%d, outputs on' % k,
          'c': '%d launches, nsub=1, no outputs' % k,
          'd': 'dmc_batch_step_n, %d steps, outputs on' % k}
  for name, _ in variants:
    lines.append('(%s) %-36s %8.2f us per physics step   (%.2f .. %.2f)' % (
        name, text[name], med[name]/k*1e3, min(ms[name])/k*1e3, max(ms[name])/k*1e3))
  lines.append('(b)/(a) = %.3f   (a)-(c) = %.2f us per step   (d)/(a) = %.3f' % (
      med['b']/med['a'], (med['a'] - med['c'])/k*1e3, med['d']/med['a']))
  lines.append('qpos after the sequence: (b) == (a): %s, (c) == (a): %s, (d) == (a): %s' % tuple(
      bool(np.array_equal(final[x], final['a'])) for x in 'bcd'))
  out = '\n'.join(lines) + '\n'
  sys.stdout.write(out)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(out)
  physics.free()


if __name__ == '__main__':
  main()
