"""Error of the device tanh that the step kernel's policy calls, in units of
u = eps(real)/2, over the hidden pre-activations of the policy cases of
tests/test_gpu_rollout.py (tests/rollout_cases.py), against a long-double tanh.

  python tools/tanh_probe.py --build        (no GPU: compiles tools/_build/tanh_probe_f32|f64)
  python tools/tanh_probe.py [--out FILE]   (on the GPU)

The programs are tools/tanh_probe.hip built with the flags of the model code
objects (build._flags), fp32 and fp64.  The figure goes into DESIGN.md 4.3 and,
doubled, into TANH_ULPS of the test.
"""

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT = os.path.join(ROOT, 'tools', '_build')


def programs(compile_them):
  import helpers
  from dm_control_amd import build
  exes = {}
  model = helpers.load_model('cartpole')
  for precision in ('f32', 'f64'):
    exe = os.path.join(OUT, 'tanh_probe_' + precision)
    exes[precision] = exe
    if compile_them:
      os.makedirs(OUT, exist_ok=True)
      spec = build.spec(model, 1, precision, None, (), 'unrolled', None, 64)
      flags = [f for f in build._flags(spec, spec.tiers[0])    # pylint: disable=protected-access
               if not f.startswith('-pragma-unroll') and f != '-mllvm']
      subprocess.check_call([build._hipcc()] + flags + [             # pylint: disable=protected-access
          '-o', exe, os.path.join(ROOT, 'tools', 'tanh_probe.hip')])
  return exes


def pre_activations(name, precision, hidden):
  """The hidden pre-activations of one policy case, as the device forms them up to
  rounding: fp64 over the recorded observations, rounded to `real`."""
  import torch
  import helpers
  import rollout_cases
  from dm_control_amd import build
  from dm_control_amd import wrapper as W
  case = rollout_cases.policy_case(name, precision, hidden)
  model = helpers.load_model(name)
  hm = W.HipModel(build.build_model(model, helpers.TASKS[name], precision, rollout=True))
  n, steps, nobs = case['nenv'], case['nsteps'], case['nobs']
  hb = W.HipBatch(hm, n)
  qpos, qvel = helpers.initial_states(model, name, n, seed=4)
  hb.set_state(qpos.T, qvel.T)
  hb.forward()
  first = hb.read(W.FIELD_OBS)
  dt = torch.float32 if precision == 'f32' else torch.float64
  obs = torch.zeros(steps, n, nobs, device='cuda', dtype=dt)
  weights = torch.from_numpy(case['policy'].packed(hm.dtype)).cuda()
  torch.cuda.synchronize()
  hb.rollout(steps, 1, policy=(weights.data_ptr(), case['policy'].widths),
             obs_out=(obs.data_ptr(), n*nobs))
  hb.sync()
  h = np.concatenate([first[None], obs.cpu().numpy()[:-1]]).astype(np.float64).reshape(-1, nobs)
  hb.free()
  hm.free()
  pre = []
  for w, b in list(zip(case['policy'].weights, case['policy'].biases))[:-1]:
    z = h @ w.astype(hm.dtype).astype(np.float64).T + b.astype(hm.dtype).astype(np.float64)
    pre.append(z.astype(hm.dtype).ravel())
    h = np.tanh(z)
  return np.concatenate(pre)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--build', action='store_true')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  exes = programs(args.build)
  if args.build:
    return
  import rollout_cases
  result = {}
  for name, precision in rollout_cases.POLICY_DOMAINS:
    x = np.concatenate([pre_activations(name, precision, hidden)
                        for hidden in rollout_cases.POLICY_HIDDEN])
    path = os.path.join(OUT, 'pre_%s.bin' % precision)
    x.tofile(path)
    count, worst, at = subprocess.check_output([exes[precision], path],
                                               universal_newlines=True).split()
    result[precision] = {'domain': name, 'values': int(count), 'max_abs_pre_activation':
                         float(np.abs(x).max()), 'max_error_in_u': float(worst), 'at': float(at)}
    os.remove(path)
  text = json.dumps(result, indent=1, sort_keys=True)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
