"""What a closed-loop rollout costs per control step, four ways.

  python tools/rollout_probe.py [--out FILE] [--batch 8192] [--steps 1000] [--warmup 100]

cheetah-run, fp32, policy 17 -> 64 -> 64 -> 6 (tanh), `--steps` control steps timed
after `--warmup`, wall clock around a device synchronisation:

  (i)   `VecEnv.step` in a loop, the policy a torch module (the path without rollouts)
  (ii)  `VecEnv.rollout` with T = 64: policy, noise and per-step records in the step kernel
  (iii) `step_device_n` over a resident action sequence on the default code object: the ceiling
  (iv)  as (ii) through `Physics.rollout_device` with rewards only (no observation record)

`--reps` alternating runs of each; the median and the spread are reported.

  python tools/rollout_probe.py --population [--members 128] [--out FILE] ...

what a population of policies costs, same workload, the legs of DESIGN.md 5:

  (i)   `VecEnv.rollout` with the shared policy on the plain rollout build
  (ii)  the population build with P = 1
  (iii) the population build with P = `--members`
  (iv)  the population build with P = the batch: one policy per env
  (v)   one policy per env without it: `VecEnv.step` in a loop, the policies a batched
        torch `bmm` over [P, B/P, .]
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
  ap.add_argument('--population', action='store_true')
  ap.add_argument('--members', type=int, default=128)
  args = ap.parse_args()
  if args.population:
    return population(args)
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


def _report(args, workload, code_objects, ms, n):
  result = dict(code_objects)
  result.update({
      'workload': workload,
      'ms_per_control_step': {
          name: {'median': float(np.median(v)), 'min': min(v), 'max': max(v), 'runs': v}
          for name, v in ms.items()},
      'env_steps_per_second': {name: n/(float(np.median(v))*1e-3) for name, v in ms.items()}})
  text = json.dumps(result, indent=1, sort_keys=True)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text + '\n')


def population(args):
  import torch
  from dm_control_amd import vec_env
  from dm_control_amd.rl import policy as policy_lib
  n, steps = args.batch, args.steps
  widths, nparams = (64, 64, 6), 17*64 + 64 + 64*64 + 64 + 64*6 + 6
  kw = dict(seed=0, torch_io=True, task_kwargs={'time_limit': float('inf')})
  plain = vec_env.VecEnv('cheetah', 'run', n, **kw)
  roll = vec_env.VecEnv('cheetah', 'run', n, rollout=True, **kw)
  pop_env = vec_env.VecEnv('cheetah', 'run', n, rollout=True, population=True, **kw)
  noise = 0.1*torch.randn(64, n, 6, device='cuda')
  gen = torch.Generator(device='cuda')
  gen.manual_seed(0)

  def resident(members):
    # N(0, 1/fan_in) weights like a fresh nn.Linear stack, in place on the device
    theta = torch.randn(nparams, members, device='cuda', generator=gen)
    at = 0
    for fan_in, out in ((17, 64), (64, 64), (64, 6)):
      theta[at:at + out*fan_in] /= fan_in**0.5
      theta[at + out*fan_in:at + out*fan_in + out] *= 0.1
      at += out*fan_in + out
    return policy_lib.MLPPopulation.from_device(theta, 17, widths)

  pops = {'ii': resident(1), 'iii': resident(args.members), 'iv': resident(n)}
  shared = pops['ii'].member(0)
  # (v): the members of (iv) as batched matrices [P, out, in]
  theta, layers, at = pops['iv'].device_tensor, [], 0
  for fan_in, out in ((17, 64), (64, 64), (64, 6)):
    w = theta[at:at + out*fan_in].T.reshape(n, out, fan_in).contiguous()
    b = theta[at + out*fan_in:at + out*fan_in + out].T.reshape(n, 1, out).contiguous()
    layers.append((w, b))
    at += out*fan_in + out

  def rollout_with(env, policy):
    def run(k):
      for t in range(0, k, 64):
        env.rollout(min(64, k - t), policy=policy, noise=noise)
    return run

  def step_loop(k):
    obs = plain._obs_t                             # pylint: disable=protected-access
    with torch.no_grad():
      for t in range(k):
        h = obs.view(n, 1, 17)
        for l, (w, b) in enumerate(layers):
          h = torch.baddbmm(b, h, w.transpose(1, 2))
          if l < 2:
            h = torch.tanh(h)
        obs, _, _, _ = plain.step(h.view(n, 6) + noise[t % 64])

  variants = (('i', rollout_with(roll, shared)), ('ii', rollout_with(pop_env, pops['ii'])),
              ('iii', rollout_with(pop_env, pops['iii'])),
              ('iv', rollout_with(pop_env, pops['iv'])), ('v', step_loop))
  for env in (plain, roll, pop_env):
    env.reset()
  ms = {name: [] for name, _ in variants}
  for _ in range(args.reps):
    for name, fn in variants:
      fn(args.warmup)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn(steps)
      torch.cuda.synchronize()
      ms[name].append((time.perf_counter() - t0)*1e3/steps)
  _report(args, 'cheetah-run, %d envs, fp32, policies 17-64-64-6, P = 1 / %d / %d, %d control '
                'steps after %d warm-up, wall clock, %d alternating runs'
          % (n, args.members, n, steps, args.warmup, args.reps),
          {'code_object_default': os.path.basename(plain.environment.physics.code_object),
           'code_object_rollout': os.path.basename(roll.environment.physics.code_object),
           'code_object_population': os.path.basename(pop_env.environment.physics.code_object)},
          ms, n)
  for env in (plain, roll, pop_env):
    env.close()


if __name__ == '__main__':
  main()
