"""Rollouts without a GPU: the build spec, `rl.policy.MLPPolicy`, and the rollout
variant of the step kernel run on the host under ASan + UBSan
(tests/host_shim/rollout_harness.cpp, a stand-alone program run directly).  The
MI355X counterpart is tests/test_gpu_rollout.py.
"""

import os
import subprocess

import numpy as np
import pytest

import helpers
import rollout_cases
import shim_runner
from dm_control_amd import build
from dm_control_amd import codegen
from dm_control_amd.rl import policy as policy_lib


# -- build.spec --------------------------------------------------------------------

def _spec(model, task, precision='f32', mode='auto', **kw):
  return build.spec(model, task, precision, None, (), mode, None, 64, **kw)


def test_spec_rollout_adds_one_flag_and_changes_the_key():
  model = helpers.load_model('cheetah')
  task = helpers.TASKS['cheetah']
  plain, default, roll = _spec(model, task), _spec(model, task, rollout=False), \
      _spec(model, task, rollout=True)
  assert plain == default and plain.flags == ()
  assert roll.flags == ('-DDMC_ROLLOUT=1',)
  assert roll.tiers == plain.tiers and roll.source == plain.source == 'dmc_kernels.hip'
  # pylint: disable=protected-access
  keys = [build._key(plain, t) for t in plain.tiers]
  assert keys == [build.model_key(model, task, 'f32', None, (), t.unroll, ()) for t in plain.tiers]
  assert not set(keys) & set(build._key(roll, t) for t in roll.tiers)
  mixed = _spec(model, task, 'mixed', rollout=True)
  assert mixed.flags == ('-DDMC_STATE_COMP=1', '-DDMC_ROLLOUT=1')
  for mode in ('unrolled', 'rolled'):
    assert _spec(model, task, mode=mode, rollout=True).flags == ('-DDMC_ROLLOUT=1',)


@pytest.mark.parametrize('mode', ['coop', 'team'])
def test_spec_rollout_refuses_the_other_kernels(mode):
  model = helpers.load_model('cheetah')
  with pytest.raises(ValueError, match='one-env-per-lane kernel'):
    _spec(model, 0 if mode == 'team' else helpers.TASKS['cheetah'], mode=mode, rollout=True)
  assert _spec(model, 0 if mode == 'team' else helpers.TASKS['cheetah'], mode=mode).flags


@pytest.mark.timeout(900)
@pytest.mark.parametrize('name,precision', [('cheetah', 'f32'), ('cartpole', 'f64')])
def test_rollout_builds_cross_compile_within_budget(name, precision):
  """No tier of the ladder is skipped for a rollout build: the first one whose
  verdict is "ok" is returned, with its record next to it."""
  model = helpers.load_model(name)
  path = build.build_model(model, helpers.TASKS[name], precision, rollout=True)
  assert build._recorded(path)[0] == 'ok'             # pylint: disable=protected-access
  assert path != build.build_model(model, helpers.TASKS[name], precision)
  with open(path, 'rb') as f:
    code = f.read()
  assert b'dmc_rollout_caps' in code              # (the capability global, rollout builds only)
  with open(build.build_model(model, helpers.TASKS[name], precision), 'rb') as f:
    assert b'dmc_rollout_caps' not in f.read()


def test_physics_refuses_rollout_where_there_is_no_one_lane_build():
  from dm_control_amd.locomotion import soccer
  from dm_control_amd.suite import common
  from dm_control_amd.suite import humanoid
  assert 'rollout' in common.PHYSICS_KWARGS
  with pytest.raises(ValueError, match='one-env-per-lane'):
    humanoid.Physics(helpers.load_model('humanoid'), batch_size=4, rollout=True)
  with pytest.raises(ValueError, match='one-env-per-lane'):
    soccer.Physics(helpers.load_model('cartpole'), batch_size=4, rollout=True)


# -- MLPPolicy ---------------------------------------------------------------------

@pytest.mark.parametrize('hidden', [(5,), (5, 64)])
def test_packing_layout_round_trip(hidden):
  p = rollout_cases.make_policy(17, hidden, 6, seed=0)
  flat = p.packed(np.float64)
  assert flat.dtype == np.float64 and flat.ndim == 1
  at, fan_in = 0, 17
  for w, b in zip(p.weights, p.biases):        # per layer W[out][in] row-major, then b[out]
    out = w.shape[0]
    assert w.shape == (out, fan_in)
    for j in (0, out - 1):
      np.testing.assert_array_equal(flat[at + j*fan_in:at + (j + 1)*fan_in], w[j])
    np.testing.assert_array_equal(flat[at + out*fan_in:at + out*fan_in + out], b)
    at += out*fan_in + out
    fan_in = out
  assert at == flat.size and p.widths == tuple(hidden) + (6,)
  q = policy_lib.MLPPolicy.unpacked(flat, 17, p.widths)
  for a, b in zip(p.weights + p.biases, q.weights + q.biases):
    np.testing.assert_array_equal(a, b)
  assert p.packed(np.float32).dtype == np.float32
  np.testing.assert_array_equal(p.packed(np.float32), flat.astype(np.float32))
  obs = np.random.RandomState(1).randn(3, 7, 17)
  h = obs
  for l, (w, b) in enumerate(zip(p.weights, p.biases)):
    h = np.einsum('...i,ji->...j', h, w) + b
    h = np.tanh(h) if l < len(hidden) else h
  np.testing.assert_allclose(p.forward(obs), h, rtol=0, atol=1e-14)
  got, bound = p.forward(obs, np.float64, 1.0)
  assert bound.shape == got.shape == (3, 7, 6) and (bound > 0).all() and bound.max() < 1e-12
  np.testing.assert_allclose(got, h, rtol=0, atol=1e-14)


def test_from_torch_against_torch_forward():
  import torch
  torch.manual_seed(0)
  nn = torch.nn
  for net in (nn.Sequential(nn.Linear(17, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(),
                            nn.Linear(64, 6)),
              nn.Sequential(nn.Linear(5, 3), nn.Tanh(), nn.Linear(3, 1, bias=False))):
    net = net.double()
    p = policy_lib.MLPPolicy.from_torch(net)
    obs = torch.randn(11, p.obs_dim, dtype=torch.float64)
    with torch.no_grad():
      want = net(obs).numpy()
    np.testing.assert_allclose(p.forward(obs.numpy()), want, rtol=0, atol=1e-14)
  with pytest.raises(ValueError, match='nn.Tanh'):
    policy_lib.MLPPolicy.from_torch(nn.Sequential(nn.Linear(5, 3), nn.ReLU(), nn.Linear(3, 1)))
  with pytest.raises(ValueError, match='linear output'):
    policy_lib.MLPPolicy.from_torch(nn.Sequential(nn.Linear(5, 3), nn.Tanh()))
  with pytest.raises(ValueError, match='1 or 2 hidden layers'):
    policy_lib.MLPPolicy.from_torch(nn.Sequential(nn.Linear(5, 1)))


def test_shape_errors_and_update():
  w = [np.zeros((3, 5)), np.zeros((2, 3))]
  b = [np.zeros(3), np.zeros(2)]
  policy_lib.MLPPolicy(w, b)
  with pytest.raises(ValueError, match='takes 4 inputs'):
    policy_lib.MLPPolicy([w[0], np.zeros((2, 4))], b)
  with pytest.raises(ValueError, match=r'biases\[0\]'):
    policy_lib.MLPPolicy(w, [np.zeros(4), b[1]])
  with pytest.raises(ValueError, match='as many bias vectors'):
    policy_lib.MLPPolicy(w, b[:1])
  with pytest.raises(ValueError, match='1 or 2 hidden layers'):
    policy_lib.MLPPolicy(w + [np.zeros((2, 2)), np.zeros((2, 2))], b + [np.zeros(2)]*2)
  with pytest.raises(ValueError, match='matrix'):
    policy_lib.MLPPolicy([np.zeros(5), w[1]], b)
  with pytest.raises(ValueError, match='values for widths'):
    policy_lib.MLPPolicy.unpacked(np.zeros(10), 5, (3, 2))
  p = policy_lib.MLPPolicy(w, b)
  assert p.version == 0
  p.update_([w[0] + 1, w[1]], b)
  assert p.version == 1 and p.weights[0][0, 0] == 1
  with pytest.raises(ValueError, match='keeps the shapes'):
    p.update_([np.zeros((4, 5)), np.zeros((2, 4))], [np.zeros(4), b[1]])


# -- the kernel on the host, under sanitizers -----------------------------------------

NENV, NSTEPS = 67, 3        # a full workgroup and a 3-env tail
RUN_TIMEOUT = 600


def _build_harness(name, tmp_path, extra=()):
  model = helpers.load_model(name)
  header = tmp_path/'model.h'
  text = codegen.generate_header(model, helpers.TASKS[name], unroll=True)
  header.write_text(text.replace('static __device__ constexpr', 'static constexpr'))
  exe = tmp_path/'rollout_harness'
  subprocess.check_call(
      ['g++', '-std=c++17', '-w', '-pthread', '-O1', '-g', '-fsanitize=address,undefined',
       '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-DDMC_REAL_IS_DOUBLE',
       '-DDMC_ROLLOUT=1'] + list(extra) + [
           '-DDMC_MODEL_HEADER="%s"' % header,
           '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(shim_runner.CSRC, 'dmc_kernels.hip'),
           '-I', shim_runner.CSRC, '-I', shim_runner.SHIM, '-x', 'c++',
           os.path.join(shim_runner.SHIM, 'rollout_harness.cpp'), '-o', str(exe)])
  return model, str(exe)


def _run(exe, model, qpos, qvel, calls, records=True, ctrl=None, policy=None):
  """-> dict: 'call' [ncalls, n, nobs + 1] (the obs and reward fields after every
  launch), 'obs' / 'reward' / 'action' (the records) and 'final' [n, ...]."""
  widths = (0, 0) if policy is None else (policy.widths[:-1] + (0,))[:2]
  text = '%d %d 1 %d %d %d %d %d %d %s\n' % (
      NENV, NSTEPS, records, ctrl is not None, 0 if policy is None else len(policy.widths) - 1,
      widths[0], widths[1], len(calls), ' '.join('%d' % c for c in calls))
  if policy is not None:
    text += ' '.join('%.17g' % x for x in policy.packed(np.float64)) + '\n'
  for e in range(NENV):
    text += ' '.join('%.17g' % x for x in np.concatenate([qpos[e], qvel[e]])) + '\n'
  if ctrl is not None:
    text += ' '.join('%.17g' % x for x in np.asarray(ctrl).ravel()) + '\n'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
  out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=RUN_TIMEOUT)
  assert out.returncode == 0, out.stderr[-3000:]
  rows = {'CALL': [], 'TRAJ': [], 'FINAL': []}
  for line in out.stdout.splitlines():
    tag, _, rest = line.partition(' ')
    rows[tag].append([float(x) for x in rest.replace('|', ' ').split()])
  nobs, nu = len(rows['CALL'][0]) - 3, model.nu
  res = {'call': np.array(rows['CALL']).reshape(len(calls), NENV, -1)[:, :, 2:],
         'final': np.array(rows['FINAL'])[:, 1:]}
  if records:
    traj = np.array(rows['TRAJ']).reshape(NSTEPS, NENV, -1)[:, :, 2:]
    assert traj.shape[2] == nobs + 1 + nu
    res.update(obs=traj[:, :, :nobs], reward=traj[:, :, nobs], action=traj[:, :, nobs + 1:])
  return res


def _same(a, b, keys=('obs', 'reward', 'action', 'final')):
  for k in keys:
    np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize('name,extra', [
    ('cheetah', ('-DDMC_LDS_BUDGET=16384',)),              # case A: rows in LDS and in the workspace
    ('cartpole', ('-DROLLOUT_EXPECT_POLICY_SIZED=1',))])   # case B: the policy sizes the LDS array
def test_rollout_kernel_on_the_host(name, extra, tmp_path):
  """fp64, 67 envs, T = 3, a two-hidden-layer policy of widths (5, 64) plus noise:
  (a) the per-step records equal the fields after single steps, (b) one launch
  equals T launches, (c) the recorded actions replay the rollout -- bit for bit."""
  model, exe = _build_harness(name, tmp_path, extra)
  qpos, qvel = helpers.initial_states(model, name, NENV, seed=7)
  nobs = {'cheetah': 17, 'cartpole': 5}[name]
  policy = rollout_cases.make_policy(nobs, (5, 64), model.nu, seed=2)
  noise = 0.3*np.random.RandomState(3).randn(NSTEPS, NENV, model.nu)
  kw = dict(ctrl=noise, policy=policy)
  one = _run(exe, model, qpos, qvel, [NSTEPS], **kw)
  each = _run(exe, model, qpos, qvel, [1]*NSTEPS, **kw)
  _same(one, each)                                                         # (b)
  assert np.isfinite(one['final']).all() and not one['final'][:, -1].any()  # (no warning bit)
  if name == 'cheetah':
    assert one['final'][:, -4].max() > 0       # (contacts: the solver ran)
  replay = _run(exe, model, qpos, qvel, [NSTEPS], ctrl=one['action'])
  _same(one, replay)                                                       # (c)
  singles = _run(exe, model, qpos, qvel, [1]*NSTEPS, records=False, ctrl=one['action'])
  np.testing.assert_array_equal(singles['call'][:, :, :nobs], one['obs'])         # (a)
  np.testing.assert_array_equal(singles['call'][:, :, nobs], one['reward'])
  np.testing.assert_array_equal(singles['final'], one['final'])
  np.testing.assert_array_equal(each['call'][:, :, :nobs], one['obs'])
  # the policy is the MLP on o_t, the record of step t-1
  want, bound = policy.forward(one['obs'][:-1], np.float64, 1.0)
  err = np.abs(one['action'][1:] - noise[1:] - want)
  assert np.all(err <= 2*bound), float((err/bound).max())
