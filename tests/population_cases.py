"""Shared by the population tests (tests/test_population_host.py,
tests/test_gpu_population.py): the population code objects the GPU tests load, seeded
populations, and the precondition that a wrong-member bug cannot pass."""

import numpy as np

import rollout_cases
from dm_control_amd.rl import policy as policy_lib

# (domain, precision) of every population build the GPU tests load
GPU_BUILDS = (('cheetah', 'f32'), ('cartpole', 'f64'))
DIMS = {'cheetah': (17, 6), 'cartpole': (5, 1)}    # (nobs, nu)


def gpu_builds():
  """[(model, task, build_model kwargs)] of every population code object the GPU tests load."""
  import helpers
  return [(helpers.load_model(d), helpers.TASKS[d],
           dict(precision=p, rollout=True, population=True)) for d, p in GPU_BUILDS]


def make_population(obs_dim, hidden, nu, members, seed):
  """`members` policies of `rollout_cases.make_policy`, seeds seed*1000 + i."""
  return policy_lib.MLPPopulation.from_policies(
      [rollout_cases.make_policy(obs_dim, hidden, nu, seed=seed*1000 + i)
       for i in range(members)])


def member_of_env(nenv, members):
  return np.arange(nenv)//(nenv//members)


def member_actions(pop, obs, dtype, tanh_ulps):
  """obs [..., nenv, nobs] -> (want, bound) [..., nenv, nu] of every env's own member,
  fp64 model with the weights rounded to `dtype`."""
  nenv = obs.shape[-2]
  group = nenv//pop.num_members
  want = np.empty(obs.shape[:-1] + (pop.action_dim,))
  bound = np.empty_like(want)
  for m in range(pop.num_members):
    sl = slice(m*group, (m + 1)*group)
    want[..., sl, :], bound[..., sl, :] = pop.member(m).forward(obs[..., sl, :], dtype, tanh_ulps)
  return want, bound


def assert_members_tell_apart(pop, obs, dtype, tanh_ulps):
  """The precondition of every test that compares an env with its member's model: on
  each env's observations, the actions of the neighbouring members (m - 1 and m + 1,
  where they exist) differ from its own member's by more than 100 times the bound in
  at least one component.  Every env, every step: none left out."""
  nenv = obs.shape[-2]
  P = pop.num_members
  if P == 1:
    return
  group = nenv//P
  for m in range(P):
    o = obs[..., m*group:(m + 1)*group, :]
    own, bound = pop.member(m).forward(o, dtype, tanh_ulps)
    for other in (m - 1, m + 1):
      if 0 <= other < P:
        theirs = pop.member(other).forward(o)
        apart = (np.abs(theirs - own) > 100*bound).any(axis=-1)
        assert apart.all(), (m, other, float((np.abs(theirs - own)/bound).max(axis=-1).min()))
