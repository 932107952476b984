"""Shared by the rollout tests (tests/test_rollout_host.py, tests/test_gpu_rollout.py):
the rollout code objects the GPU tests load, and seeded policies."""

import numpy as np

from dm_control_amd.rl import policy as policy_lib

# (domain, precision) of every rollout build the GPU tests load
GPU_BUILDS = (('cheetah', 'f32'), ('hopper', 'f32'), ('cartpole', 'f64'),
              ('cheetah', 'mixed'), ('cheetah', 'f64'))


def gpu_builds():
  """[(model, task, build_model kwargs)] of every rollout code object the GPU tests load."""
  import helpers
  return [(helpers.load_model(d), helpers.TASKS[d], dict(precision=p, rollout=True))
          for d, p in GPU_BUILDS]


POLICY_DOMAINS = (('cheetah', 'f32'), ('cartpole', 'f64'))
POLICY_HIDDEN = ((3,), (64,), (3, 64), (64, 3))     # one and two hidden layers, widths 3 and 64
_DIMS = {'cheetah': (17, 6), 'cartpole': (5, 1)}    # (nobs, nu)


def policy_case(name, precision, hidden):
  """A case of the test that the device policy computes the MLP (70 envs: a full
  workgroup and a tail; 3 steps), also what tools/tanh_probe.py measures over."""
  del precision
  nobs, nu = _DIMS[name]
  return dict(nenv=70, nsteps=3, nu=nu, nobs=nobs,
              policy=make_policy(nobs, hidden, nu, seed=10 + len(hidden) + hidden[0]))


def make_policy(obs_dim, hidden, nu, seed, scale=1.0):
  """An MLP with weights ~ N(0, scale^2/fan_in) and biases ~ N(0, 0.1^2): hidden
  pre-activations of order one, so tanh is exercised on both of its branches."""
  rs = np.random.RandomState(seed)
  weights, biases, fan_in = [], [], obs_dim
  for out in tuple(hidden) + (nu,):
    weights.append(scale*rs.randn(out, fan_in)/np.sqrt(fan_in))
    biases.append(0.1*rs.randn(out))
    fan_in = out
  return policy_lib.MLPPolicy(weights, biases)
