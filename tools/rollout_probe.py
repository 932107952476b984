"""What a closed-loop rollout costs per control step, four ways.

  python tools/rollout_probe.py [--out FILE] [--batch 8192] [--steps 1000] [--warmup 100]

cheetah-run, fp32, policy 17 -> 64 -> 64 -> 6 (tanh), `--steps` control steps timed
after `--warmup`, wall clock around a device synchronisation:

  (i)   `VecEnv.step` in a loop, the policy a torch module (the path without rollouts)
  (ii)  `VecEnv.rollout` with T = 64: policy, noise and per-step records in the step kernel
  (iii) `step_device_n` over a resident action sequence on the default code object: the ceiling
  (iv)  as (ii) through `Physics.rollout_device` with rewards only (no observation record)

`--reps` alternating runs of each; the median and the spread are reported.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--batch', type=int, default=8192)
  ap.add_argument('--steps', type=int, default=1000)
  ap.add_argument('--warmup', type=int, default=100)
  ap.add_argument('--reps', type=int, default=6)
  args = ap.parse_args()
  import torch
  from dm_control_amd import vec_env
  from dm_control_amd.rl import policy as policy_lib
  n, steps = args.batch, args.steps
  torch.manual_seed(0)
  net = torch.nn.Sequential(torch.nn.Linear(17, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64),
                            torch.nn.Tanh(), torch.nn.Linear(64, 6)).cuda()
  policy = policy_lib.MLPPolicy.from_torch(net)
  kw = dict(seed=0, torch_io=True, task_kwargs={'time_limit': float('inf')})
  plain = vec_env.VecEnv('cheetah', 'run', n, **kw)
  roll = vec_env.VecEnv('cheetah', 'run', n, rollout=True, **kw)
  noise = 0.1*torch.randn(64, n, 6, device='cuda')
  acts = torch.rand(64, n, 6, device='cuda')*2 - 1
  rewards = torch.empty(64, n, device='cuda')
  packed = torch.from_numpy(policy.packed(np.float32)).cuda()

  def step_loop(k):
    obs = plain._obs_t                             # pylint: disable=protected-access
    with torch.no_grad():
      for t in range(k):
        obs, _, _, _ = plain.step(net(obs) + noise[t % 64])

  def rollout(k):
    for t in range(0, k, 64):
      roll.rollout(min(64, k - t), policy=policy, noise=noise)

  def open_loop(k):
    batch = plain._batch                           # pylint: disable=protected-access
    for t in range(0, k, 64):
      batch.step_device_n(acts.data_ptr(), 1, 6, n*6, min(64, k - t), 1)

  def rewards_only(k):
    physics = roll._physics                        # pylint: disable=protected-access
    for t in range(0, k, 64):
      physics.rollout_device(min(64, k - t), 1, ctrl=(noise.data_ptr(), 1, 6, n*6),
                             policy=(packed.data_ptr(), policy.widths),
                             reward_out=(rewards.data_ptr(), n))

  variants = (('i', step_loop), ('ii', rollout), ('iii', open_loop), ('iv', rewards_only))
  plain.reset()
  roll.reset()
  ms = {name: [] for name, _ in variants}
  for rep in range(args.reps):
    for name, fn in variants:
      fn(args.warmup)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn(steps)
      torch.cuda.synchronize()
      ms[name].append((time.perf_counter() - t0)*1e3/steps)
  result = {
      'workload': 'cheetah-run, %d envs, fp32, policy 17-64-64-6, %d control steps after %d '
                  'warm-up, wall clock, %d alternating runs' % (n, steps, args.warmup, args.reps),
      'code_object_default': os.path.basename(plain.environment.physics.code_object),
      'code_object_rollout': os.path.basename(roll.environment.physics.code_object),
      'ms_per_control_step': {
          name: {'median': float(np.median(v)), 'min': min(v), 'max': max(v), 'runs': v}
          for name, v in ms.items()},
      'env_steps_per_second': {name: n/(float(np.median(v))*1e-3) for name, v in ms.items()},
  }
  text = json.dumps(result, indent=1, sort_keys=True)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text + '\n')
  plain.close()
  roll.close()


if __name__ == '__main__':
  main()
