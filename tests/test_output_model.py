"""The host model of the output stage (tests/output_model.py) pinned on the CPU:
against the fp64 oracle, against the goldens of the reference, and the
conditions on the case states (tests/output_cases.py) that the device tests
(tests/test_gpu_outputs.py) rely on.  The kernel sources are compared with the
model on the host in tests/test_kernel_sanitizers.py (observe mode of the shim).
"""

import functools
import json
import os

import numpy as np
import pytest

import helpers
import output_cases as cases
import output_model as M
import task_formulas
from dm_control_amd import codegen
from dm_control_amd.utils import rewards
from oracle import oracle

VARIANTS = [(d,) + v for d in cases.DOMAINS for v in cases.VARIANTS[d]]
IDS = ['%s-%s' % v[:2] for v in VARIANTS]


@functools.lru_cache(maxsize=None)
def _states(domain, poles):
  return cases.states(domain, poles)


@functools.lru_cache(maxsize=None)
def _evaluated(domain, label, dtype=np.float64):
  _, poles, param_i, param_r = next(v for v in cases.VARIANTS[domain] if v[0] == label)
  model, qpos, qvel, ctrl, taskdata = _states(domain, poles)
  return M.evaluate(model, helpers.TASKS[domain], param_i, param_r, qpos, qvel, ctrl,
                    taskdata, dtype)


def _golden(name):
  with open(os.path.join(helpers.GOLDEN, name)) as f:
    return json.load(f)


# --------------------------------------------------------------------------
# (a) model vs oracle
# --------------------------------------------------------------------------
@pytest.mark.parametrize('domain,poles', sorted(
    {(v[0], v[2]) for v in VARIANTS}, key=str), ids=str)
def test_model_matches_oracle(domain, poles):
  """Frames, subtree quantities and the non-touch sensors of every case state,
  to the 1e-12 of test_derived_frames_match_oracle.  The oracle (as the
  reference) runs the subtree-velocity pass only for models that declare such a
  sensor; for the others the expected value is the mass-weighted mean of the
  oracle's own velocities of the bodies' centres of mass."""
  model, qpos, qvel, ctrl, taskdata = _states(domain, poles)
  label = next(v[1] for v in VARIANTS if v[0] == domain and v[2] == poles)
  out = _evaluated(domain, label)
  om = oracle.OracleModel(model)
  d = oracle.OracleData(om)
  has_linvel = (np.asarray(model.sensor_type) == 35).any() if model.nsensor else False
  nb = int(model.nbody)
  modelled = ~np.isnan(out.sensordata[0])
  assert modelled.sum() == sum(int(model.sensor_dim[s]) for s in range(int(model.nsensor))
                               if int(model.sensor_type[s]) in (8, 9, 34, 35))
  for i in range(len(qpos)):
    d.qpos[:], d.qvel[:], d.ctrl[:] = qpos[i], qvel[i], ctrl[i]
    d.step1()
    for name in ('xpos', 'xmat', 'xipos', 'subtree_com'):
      np.testing.assert_allclose(getattr(out, name)[i], getattr(d, name), rtol=0, atol=1e-12,
                                 err_msg='%s of env %d' % (name, i))
    if has_linvel:
      want = d.subtree_linvel
    else:
      want = np.array([model.body_mass[b]*d.point_velocity(b, d.xipos[b])[0]
                       for b in range(nb)])
      for b in range(nb - 1, 0, -1):
        want[int(model.body_parentid[b])] += want[b]
      want /= np.maximum(1e-15, np.asarray(model.body_subtreemass))[:, None]
    np.testing.assert_allclose(out.subtree_linvel[i], want, rtol=0, atol=1e-12,
                               err_msg='subtree_linvel of env %d' % i)
    if modelled.any():
      np.testing.assert_allclose(out.sensordata[i, modelled], d.sensordata[modelled],
                                 rtol=0, atol=1e-12)


# --------------------------------------------------------------------------
# (b) model vs goldens
# --------------------------------------------------------------------------
def test_dtype_honouring_tolerance_is_the_products():
  """task_formulas.tolerance against utils.rewards.tolerance (pinned by
  rewards.json) on the golden grid, and the goldens themselves."""
  seen = 0
  for g in _golden('rewards.json'):
    if g['sigmoid'] not in ('gaussian', 'linear', 'quadratic'):
      continue
    bounds = tuple(float(b) for b in g['bounds'])
    kw = dict(bounds=bounds, margin=g['margin'], sigmoid=g['sigmoid'],
              value_at_margin=g['value_at_margin'])
    x = np.array(g['x'])
    got = task_formulas.tolerance(x, **kw)
    np.testing.assert_array_equal(got, rewards.tolerance(x, **kw))
    np.testing.assert_allclose(got, g['y'], rtol=1e-14, atol=1e-300)
    got32 = task_formulas.tolerance(x.astype(np.float32), **kw)
    assert got32.dtype == np.float32
    seen += 1
  assert seen >= 10


def test_rewards_on_the_golden_records_through_the_model():
  """Every tasks.json record through the functions `evaluate` calls, batched
  (env on the leading axis) as `evaluate` calls them, in float64 and float32."""
  g = _golden('tasks.json')
  col = lambda recs, key: np.array([r[key] for r in recs])
  checks = []
  r = g['cartpole']
  for sparse, key in ((False, 'reward_smooth'), (True, 'reward_sparse')):
    checks.append((lambda dt, sparse=sparse: task_formulas.cartpole_reward(
        col(r, 'x').astype(dt), col(r, 'cos').astype(dt)[:, None],
        col(r, 'ctrl').astype(dt)[:, None], col(r, 'qvel').astype(dt)[:, 1:], sparse),
                   col(r, key)))
  r2 = g['cheetah']
  checks.append((lambda dt: task_formulas.cheetah_reward(col(r2, 'speed').astype(dt)),
                 col(r2, 'reward')))
  r3 = g['humanoid']
  for speed in (0, 1, 10):
    checks.append((lambda dt, speed=speed: task_formulas.humanoid_reward(
        col(r3, 'head_height').astype(dt), col(r3, 'torso_upright').astype(dt),
        col(r3, 'ctrl').astype(dt), col(r3, 'com_velocity').astype(dt), float(speed)),
                   col(r3, 'reward_speed_%d' % speed)))
  r4 = g['walker']
  for speed in (0, 1, 8):
    checks.append((lambda dt, speed=speed: task_formulas.walker_reward(
        col(r4, 'torso_height').astype(dt), col(r4, 'torso_upright').astype(dt),
        col(r4, 'horizontal_velocity').astype(dt), float(speed)),
                   col(r4, 'reward_speed_%d' % speed)))
  r5 = g['pendulum']
  checks.append((lambda dt: task_formulas.pendulum_reward(col(r5, 'pole_vertical').astype(dt)),
                 col(r5, 'reward')))
  r6 = g['acrobot']
  for sparse, key in ((False, 'reward_smooth'), (True, 'reward_sparse')):
    checks.append((lambda dt, sparse=sparse: task_formulas.acrobot_reward(
        col(r6, 'to_target').astype(dt), sparse, target_radius=dt(0.2)), col(r6, key)))
  r7 = g['hopper']
  for hopping, key in ((False, 'reward_stand'), (True, 'reward_hop')):
    checks.append((lambda dt, hopping=hopping: task_formulas.hopper_reward(
        col(r7, 'height').astype(dt), col(r7, 'speed').astype(dt),
        col(r7, 'ctrl').astype(dt), hopping), col(r7, key)))
  r8 = g['reacher']
  for size in (0.05, 0.015):
    checks.append((lambda dt, size=size: task_formulas.reacher_reward(
        col(r8, 'dist').astype(dt), dt(size + 0.01), finger_size=dt(0)),
                   col(r8, 'reward_%g' % size)))
  r9 = g['point_mass']
  checks.append((lambda dt: task_formulas.point_mass_reward(
      col(r9, 'dist').astype(dt), col(r9, 'ctrl').astype(dt), target_size=dt(0.015)),
                 col(r9, 'reward')))
  for fn, want in checks:
    got = fn(np.float64)
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-300)
    got32 = fn(np.float32)
    assert got32.dtype == np.float32
    # canned readings are far from the margin-0 bounds: float32 keeps every branch
    np.testing.assert_allclose(got32, want, rtol=0, atol=2e-5)


OBS_LAYOUT, obs_slices = M.OBS_LAYOUT, M.obs_slices


@pytest.mark.parametrize('domain', cases.DOMAINS)
def test_observation_layout(domain):
  """Key order and slices of the flat observation: widths add up to the
  kernel's NOBS, the keys that copy the state are the model's `state` entries
  and hold exactly those values, and the goldens that hold observations
  (cartpole, acrobot) agree with the model's order."""
  label = cases.VARIANTS[domain][0][0]
  out = _evaluated(domain, label)
  model, qpos, qvel, _, _ = _states(domain, None)
  sl = obs_slices(domain)
  assert sum(w for _, w in OBS_LAYOUT[domain]) == out.obs.shape[1]
  assert out.obs.shape[1] == codegen.observation_size(model, helpers.TASKS[domain])
  kinds = np.array(out.obs_kinds)
  np.testing.assert_array_equal(out.obs[:, sl['velocity']],
                                qvel[:, :1] if domain == 'pendulum' else qvel)
  assert (kinds[sl['velocity']] == 'state').all()
  if domain in ('cheetah', 'hopper'):
    np.testing.assert_array_equal(out.obs[:, sl['position']], qpos[:, 1:])
  if domain in ('reacher', 'point_mass'):
    np.testing.assert_array_equal(out.obs[:, sl['position']], qpos)
  if domain == 'humanoid':
    np.testing.assert_array_equal(out.obs[:, sl['joint_angles']], qpos[:, 7:])
    assert (kinds[sl['com_velocity']] == 'vel').all()
    assert (kinds[sl['extremities']] == 'pos').all()
    torso = model.name2id('torso', 'body')
    np.testing.assert_array_equal(out.obs[:, sl['torso_vertical']], out.xmat[:, torso, 6:])
    np.testing.assert_array_equal(out.obs[:, sl['com_velocity']], out.subtree_linvel[:, torso])
  if domain == 'hopper':
    assert np.isnan(out.obs[:, sl['touch']]).all() and (kinds[sl['touch']] == 'touch').all()
  g = _golden('tasks.json')
  if domain in g['observations']:
    # the reference's get_observation on stub physics with canned readings: key
    # order, widths, and the reading every key takes
    rec = g['observations'][domain]
    assert tuple(rec['keys']) == tuple(k for k, _ in OBS_LAYOUT[domain])
    assert tuple(len(rec['values'][k]) for k in rec['keys']) == tuple(
        w for _, w in OBS_LAYOUT[domain])
    source = {'joint_angles': 'joint_angles', 'head_height': 'head_height',
              'extremities': 'extremities', 'torso_vertical': 'torso_vertical_orientation',
              'com_velocity': 'center_of_mass_velocity', 'velocity': 'velocity',
              'orientations': 'orientations', 'height': 'torso_height',
              'orientation': 'pole_orientation', 'touch': 'touch', 'position': 'position',
              'to_target': 'finger_to_target'}
    for key in rec['keys']:
      if key == 'position' and domain in ('cheetah', 'hopper'):
        assert rec['values'][key] == rec['readings']['qpos'][1:]     # without rootx
      elif key == 'velocity' and domain == 'pendulum':
        assert rec['values'][key] == rec['readings']['angular_velocity']
      else:
        assert rec['values'][key] == rec['readings'][source[key]], key
  if domain == 'humanoid':
    rec = g['observations']['humanoid_pure_state']
    assert rec['keys'] == ['position', 'velocity']
    assert [len(rec['values'][k]) for k in rec['keys']] == [model.nq, model.nv]
  if domain == 'cartpole':
    r = g['cartpole'][0]
    assert tuple(r['obs_keys']) == tuple(k for k, _ in OBS_LAYOUT[domain])
    assert len(r['obs_position']) == 3 and len(r['obs_velocity']) == 2
    # [x, cos, sin]: cos is the pole's zz, sin its xz
    pole = 2
    np.testing.assert_array_equal(out.obs[:, :3], np.stack(
        [qpos[:, 0], out.xmat[:, pole, 8], out.xmat[:, pole, 2]], axis=1))
    np.testing.assert_allclose(out.obs[:, 1], np.cos(qpos[:, 1]), atol=1e-15)
    np.testing.assert_allclose(out.obs[:, 2], np.sin(qpos[:, 1]), atol=1e-15)
  if domain == 'acrobot':
    r = g['acrobot'][0]
    assert tuple(r['obs_keys']) == tuple(k for k, _ in OBS_LAYOUT[domain])
    assert r['obs_orientations'] == r['horizontal'] + r['vertical']
    upper, lower = codegen.task_bodies(model, helpers.TASKS[domain])
    np.testing.assert_array_equal(out.obs[:, :4], np.stack(
        [out.xmat[:, upper, 2], out.xmat[:, lower, 2], out.xmat[:, upper, 8],
         out.xmat[:, lower, 8]], axis=1))


# --------------------------------------------------------------------------
# (c) coverage and exclusion
# --------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS, ids=IDS)
def test_case_states_reach_every_branch(variant):
  domain, label = variant[:2]
  out = _evaluated(domain, label)
  assert len(out.reward) == cases.NENV == 129
  hits = cases.coverage(out)
  need = cases.reachable(out)
  assert need, 'a reward without tolerance terms'
  short = {pair: hits.get(pair, 0) for pair in need if hits.get(pair, 0) < cases.MIN_HITS}
  assert not short, short
  assert set(hits) <= need, set(hits) - need
  assert np.all((out.reward >= 0) & (out.reward <= 1))
  for name in ('xpos', 'xmat', 'obs'):
    value = getattr(out, name)
    assert np.isfinite(value[~np.isnan(value)]).all()


@pytest.mark.parametrize('variant', VARIANTS, ids=IDS)
def test_case_states_leave_no_reward_sample_out(variant):
  """No margin-0 input within its own fp32 tolerance of a bound (so none within
  the much smaller fp64 one), and the float32 model takes the branches of the
  float64 model in every term."""
  domain, label = variant[:2]
  out = _evaluated(domain, label)
  assert not M.excluded(out, M.fp32_tolerances(out)).any()
  out32 = _evaluated(domain, label, np.float32)
  for a, b in zip(out.terms, out32.terms):
    if a.bounds is not None:
      np.testing.assert_array_equal(a.branch, b.branch, err_msg=a.name)


# --------------------------------------------------------------------------
# (d) the fp32 figures
# --------------------------------------------------------------------------
def measured_figures(out64, out32):
  """{class: largest |out32 - out64| / (eps32 * scale)}; the `state` class must
  be exact."""
  s = M.scales(out64)
  by64, by32 = M.classes(out64), M.classes(out32)
  fig = {}
  for kind in M.CLASSES:
    for (name, a), (_, b) in zip(by64[kind], by32[kind]):
      err = np.abs(a - b.astype(np.float64)).max(axis=1)/(M.EPS32*s[kind])
      fig[kind] = max(fig.get(kind, 0.0), float(err.max()))
  for (name, a), (_, b) in zip(by64['state'], by32['state']):
    np.testing.assert_array_equal(a.astype(np.float32), b, err_msg=name)
  return fig


def test_fp32_figures():
  """CPU_FIGURE of output_model.py, recomputed: the float32 model against the
  float64 model over all case states of all variants."""
  fig = {}
  for domain, label in [v[:2] for v in VARIANTS]:
    out32 = _evaluated(domain, label, np.float32)
    assert all(v.dtype == np.float32 for v in (
        out32.xpos, out32.xmat, out32.xipos, out32.subtree_com, out32.subtree_linvel,
        out32.obs, out32.reward, out32.sensordata))
    for kind, value in measured_figures(_evaluated(domain, label), out32).items():
      fig[kind] = max(fig.get(kind, 0.0), value)
  print('MEASURED fp32 model vs fp64 model, eps32*scale:', {k: round(v, 2) for k, v in fig.items()})
  for kind in M.CLASSES:
    assert M.CPU_FIGURE[kind]/2 <= fig[kind] <= 2*M.CPU_FIGURE[kind], (kind, fig[kind])
