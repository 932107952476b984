"""The host model of the device-side initialiser (tests/device_init_model.py)
draws what the reference's `initialize_episode` recipes state (CPU).  The
kernel is compared with the model value by value elsewhere (host shim:
tests/test_kernel_sanitizers.py; MI355X: tests/test_gpu_device_init.py), so a
distribution that fails here is a fault of the recipe both implement.

N = 65536 envs per task under fixed seeds, so every outcome is deterministic.
Bounds: one-sample Kolmogorov-Smirnov D < 2.69/sqrt(N), the alpha = 1e-6
critical value sqrt(-ln(alpha/2)/2); two-sample 2.69 sqrt(2/N); Pearson
|r| < 5/sqrt(N).
"""

import itertools
import math

import numpy as np
import pytest

import device_init_model as M
from dm_control_amd import codegen
from dm_control_amd.mjcf import model as mdl
from dm_control_amd.suite import base
from dm_control_amd.suite import randomizers

N = 65536
SEED = 20261
KS1 = 2.69/math.sqrt(N)
KS2 = 2.69*math.sqrt(2.0/N)
RMAX = 5/math.sqrt(N)
_erf = np.vectorize(math.erf)

TASK_OF = {'cartpole': codegen.TASK_CARTPOLE, 'cheetah': codegen.TASK_CHEETAH,
           'humanoid': codegen.TASK_HUMANOID, 'walker': codegen.TASK_WALKER,
           'pendulum': codegen.TASK_PENDULUM, 'acrobot': codegen.TASK_ACROBOT,
           'hopper': codegen.TASK_HOPPER, 'reacher': codegen.TASK_REACHER,
           'point_mass': codegen.TASK_POINTMASS}


def _ks(x, cdf):
  x = np.sort(np.asarray(x, np.float64))
  f = cdf(x)
  i = np.arange(1, len(x) + 1)
  return max(np.max(i/len(x) - f), np.max(f - (i - 1)/len(x)))


def _ks2(a, b):
  a, b = np.sort(a), np.sort(b)
  both = np.concatenate([a, b])
  return np.max(np.abs(np.searchsorted(a, both, side='right')/len(a) -
                       np.searchsorted(b, both, side='right')/len(b)))


def _uniform(lo, hi):
  return lambda x: np.clip((x - lo)/(hi - lo), 0, 1)


def _normal(mu, sigma):
  return lambda x: 0.5*(1 + _erf((x - mu)/(sigma*math.sqrt(2))))


def _stated(model, domain, param):
  """{qpos column: cdf}, {qvel column: cdf} and the quaternion columns, as the
  reference's recipe of the task states them (the citations are in
  tests/device_init_model.py); columns not named keep qpos0 / zero."""
  qpos, qvel, quat = {}, {}, []
  if domain == 'cartpole':
    if param & 2:
      qpos = {0: _normal(0, 0.01), 1: _normal(np.pi, 0.01)}
      qpos.update({i: _normal(0, 0.1) for i in range(2, model.nq)})
    else:
      qpos = {0: _uniform(-0.1, 0.1)}
      qpos.update({i: _uniform(-0.034, 0.034) for i in range(1, model.nq)})
    qvel = {i: _normal(0, 0.01) for i in range(model.nv)}
    return qpos, qvel, quat
  for j in range(model.njnt):
    kind, adr = int(model.jnt_type[j]), int(model.jnt_qposadr[j])
    if model.jnt_limited[j] and kind in (mdl.JNT_HINGE, mdl.JNT_SLIDE):
      qpos[adr] = _uniform(*model.jnt_range[j])
    elif domain != 'cheetah' and not model.jnt_limited[j]:
      if kind == mdl.JNT_HINGE:
        qpos[adr] = _uniform(-np.pi, np.pi)
      elif kind == mdl.JNT_FREE:
        quat += list(range(adr + 3, adr + 7))
  return qpos, qvel, quat


class _Task(base.Task):
  def get_observation(self, physics):
    raise NotImplementedError


@pytest.fixture(scope='module', params=M.CASES, ids=[c[0] for c in M.CASES])
def case(request):
  label, domain, poles, param = request.param
  model = M.case_model(domain, poles)
  task = TASK_OF[domain]
  a, b = M.product_seeds(1, 2)
  t = _Task(random=1)
  assert [t.device_seed(), t.device_seed()] == [a, b]       # what the product hands over
  draws = {s: M.draw(model, task, param, s, N) for s in (SEED, SEED + 1, a, b)}
  return label, domain, model, param, draws, (a, b)


def _columns(d, qvel_cols):
  """Every randomised coordinate of a draw, [N, columns], and the groups of
  columns that one normalisation ties together."""
  cols = [d.qpos[:, c] for c in d.randomised] + [d.qvel[:, c] for c in qvel_cols]
  tied = [i for i, c in enumerate(d.randomised) if d.tscale['qpos'][c] == 1.0]
  if d.taskdata is not None and d.tscale['taskdata'].any():
    cols += list(d.taskdata.T)
  return np.array(cols, np.float64).T, tied


def test_randomised_coordinates_follow_the_stated_distributions(case):
  label, domain, model, param, draws, _ = case
  d = draws[SEED]
  qpos, qvel, quat = _stated(model, domain, param)
  assert sorted(d.randomised) == sorted(list(qpos) + quat), 'the set of randomised coordinates'
  for c, cdf in qpos.items():
    assert _ks(d.qpos[:, c], cdf) < KS1, (label, 'qpos', c)
  for c, cdf in qvel.items():
    assert _ks(d.qvel[:, c], cdf) < KS1, (label, 'qvel', c)
  # everything else is qpos0 / zero, exactly: a free joint's translation, unlimited
  # sliders, the cheetah's unlimited root joints
  still = [c for c in range(model.nq) if c not in qpos and c not in quat]
  np.testing.assert_array_equal(d.qpos[:, still], np.tile(model.qpos0[still], (N, 1)))
  np.testing.assert_array_equal(d.qvel[:, [c for c in range(model.nv) if c not in qvel]], 0)
  for f in ('warm', 'ctrl', 'time', 'episode_return'):
    assert not getattr(d, f).any()
  if domain == 'cheetah':
    assert still == [0, 1, 2]
  if domain == 'reacher':
    # reacher.py:95-98: (r sin a, r cos a), r uniform on [0.05, 0.2], a uniform
    x, y = d.taskdata.T
    assert _ks(np.hypot(x, y), _uniform(0.05, 0.2)) < KS1
    assert _ks(np.arctan2(x, y) % (2*np.pi), _uniform(0, 2*np.pi)) < KS1
  if label == 'point_mass_easy':
    np.testing.assert_array_equal(d.taskdata, np.tile(model.wrap_prm[:4], (N, 1)))


def test_free_joint_quaternion_is_rand4_normalised(case):
  label, domain, model, param, draws, _ = case
  quat = _stated(model, domain, param)[2]
  if not quat:
    assert domain != 'humanoid'
    return
  rs = np.random.RandomState(99)
  ref = np.empty((N, model.nq))
  for row in ref:
    row[:] = model.qpos0
    randomizers.randomize_limited_and_rotational_joints(model, row, rs)
  d = draws[SEED]
  for c in quat:
    assert _ks2(d.qpos[:, c], ref[:, c]) < KS2, c
  np.testing.assert_allclose(np.linalg.norm(d.qpos[:, quat], axis=1), 1, rtol=0, atol=4e-16)
  assert d.qpos[:, quat].min() >= 0       # the positive orthant, as in the reference


def test_draws_are_independent_across_coordinates_envs_and_seeds(case):
  label, domain, model, param, draws, (a, b) = case
  qvel_cols = list(_stated(model, domain, param)[1])
  x, tied = _columns(draws[SEED], qvel_cols)
  r = np.corrcoef(x.T).reshape(x.shape[1], x.shape[1])
  for i, j in itertools.combinations(range(x.shape[1]), 2):
    if i in tied and j in tied:
      continue        # components of one unit quaternion: squares sum to one
    assert abs(r[i, j]) < RMAX, (label, 'coordinates', i, j, r[i, j])
  for k in range(x.shape[1]):
    assert abs(np.corrcoef(x[:-1, k], x[1:, k])[0, 1]) < RMAX, (label, 'env e and e+1', k)
  for s, t in ((SEED, SEED + 1), (a, b)):
    x, _ = _columns(draws[s], qvel_cols)
    y, _ = _columns(draws[t], qvel_cols)
    for k in range(x.shape[1]):
      assert abs(np.corrcoef(x[:, k], y[:, k])[0, 1]) < RMAX, (label, 'seeds', s, t, k)
    # env e of the next seed is no other env of this one either
    for k in range(x.shape[1]):
      assert abs(np.corrcoef(x[1:, k], y[:-1, k])[0, 1]) < RMAX, (label, 'seed s+1 env e, seed s env e+1', k)


def test_no_two_envs_start_alike(case):
  label, domain, model, param, draws, _ = case
  for d in draws.values():
    distinct = len(np.unique(d.qpos, axis=0))
    if len(d.randomised) == 1 and d.tscale['qpos'].sum() == 0:
      # the pendulum: ONE 24-bit uniform per row, so 65536 rows on a grid of
      # 2^24 values repeat by the birthday count alone: lambda = N (N - 1)/2^25
      # = 128 pairs expected; allowed: lambda + 5 sqrt(lambda).  (A stuck
      # counter or key would repeat thousands of rows.)
      lam = N*(N - 1)/2.0**25
      assert N - distinct <= lam + 5*math.sqrt(lam), (label, N - distinct)
    else:
      # two or more draws per row (48 bits): a repeat has probability 1e-5
      assert distinct == N, (label, N - distinct)
  rows = [np.concatenate([d.qpos, d.qvel], axis=1) for d in draws.values()]
  for x, y in itertools.combinations(rows, 2):
    assert (x != y).any(axis=1).mean() > 0.99, label


def test_point_mass_hard_directions(case):
  label, domain, model, param, draws, _ = case
  if label != 'point_mass_hard':
    return
  d = draws[SEED]
  d1, d2 = d.taskdata[:, :2], d.taskdata[:, 2:]
  np.testing.assert_allclose(np.linalg.norm(d1, axis=1), 1, rtol=0, atol=4e-16)
  np.testing.assert_allclose(np.linalg.norm(d2, axis=1), 1, rtol=0, atol=4e-16)
  assert np.abs((d1*d2).sum(axis=1)).max() <= 0.9
  assert np.abs(d1.mean(axis=0)).max() < 5/math.sqrt(N)
  # randn(2) normalised: the direction's angle is uniform
  assert _ks(np.arctan2(d1[:, 1], d1[:, 0]), _uniform(-np.pi, np.pi)) < KS1
  # the rejection drew again for the share of candidates it must: P(|cos| > 0.9)
  # (two joints, two normals for d1, two per candidate: 2 + 4 + 4k draws)
  extra = (d.draws.astype(np.int64) - 10)//4
  assert abs((extra > 0).mean() - 2*math.acos(0.9)/math.pi) < 5/math.sqrt(N)


def test_generator_is_the_documented_one():
  """Known answers from the contract computed with Python ints (not numpy):
  key, counter, finaliser, 24 bits."""
  mask = 2**64 - 1

  def mix(x):
    x ^= x >> 33
    x = x*0xff51afd7ed558ccd & mask
    x ^= x >> 33
    x = x*0xc4ceb9fe1a85ec53 & mask
    x ^= x >> 33
    return (x >> 16) & 0xffffffff
  for seed in M.SEEDS + (2**64 - 1,):
    rng = M.Rng(seed, 70)
    for c in (1, 2, 3):
      u = rng.uniform()
      for e in (0, 1, 69):
        key = (seed*0x2545F4914F6CDD1D + e) & mask
        assert u[e] == (mix((key + 0x9e3779b97f4a7c15*c) & mask) >> 8)/2.0**24
      assert u.min() >= 0 and u.max() < 1
  u = M.Rng(SEED, N).uniform()
  assert np.all(u*2**24 == np.round(u*2**24))
  z = M.Rng(SEED, N).normal()
  assert _ks(z, _normal(0, 1)) < KS1


def test_no_compared_case_sits_on_a_branch_and_the_rounding_figures_hold():
  """Part of the tolerance: in the float64 model no env of any case compared
  with a device has a point_mass candidate within 1e-4 of the 0.9 threshold or
  normalises a vector shorter than 1e-3, so no env is left out of a comparison;
  and what rounding alone does to the formulas is what device_init_model
  records (its device bound is four times that)."""
  cases = M.compared_cases(130)
  for c in cases:
    d = M.draw(*c)
    assert d.min_margin >= 1e-4 and d.min_norm >= 1e-3, (c[1:4], d.min_margin, d.min_norm)
    for real in (np.float32, np.longdouble):       # the decisions do not move with the precision
      np.testing.assert_array_equal(M.draw(*c, dtype=real).draws, d.draws)
  for real, size in ((np.float32, 4), (np.float64, 8)):
    for kind in M.KINDS:
      figure = M.rounding_figure(cases, real, kind)
      print('rounding figure of %s, %s: %.1f eps*scale' % (real.__name__, kind, figure))
      assert 0.9*M.CPU_ROUNDING_FIGURE[size][kind] <= figure <= M.CPU_ROUNDING_FIGURE[size][kind]
      assert M.bound_in_eps(size, kind) == max(8, 4*M.CPU_ROUNDING_FIGURE[size][kind])
      # ... and far below what a wrong draw is off by: the scale itself, 1/eps in this unit
      assert M.bound_in_eps(size, kind) < 1e-3/np.finfo(real).eps
