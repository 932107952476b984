"""Rollouts in one launch (`dmc_batch_rollout` on a rollout build of the
one-env-per-lane kernel): per-step outputs, the device MLP policy, the refusals and
`VecEnv.rollout`.  Every "equal" is bitwise, over the fields of
tests/test_gpu_step_sequence.py and the three recorded trajectories; all runs
inside one test use the same rollout code object.
"""

import numpy as np
import pytest
import torch

import helpers
import rollout_cases
import test_gpu_step_sequence as seq
from dm_control_amd import build
from dm_control_amd import wrapper

pytestmark = pytest.mark.gpu

W = wrapper
FIELDS = seq.FIELDS
TRAJECTORIES = ('obs_out', 'reward_out', 'action_out')
# Error of the device tanh in units of u = eps/2 of `real`, 2x the largest seen by
# tools/tanh_probe.py on the MI355X over the hidden pre-activations of the cases of
# `test_the_policy_computes_the_mlp` against a long-double tanh:
# measured 1.465 u (fp32, the project's fp32 flags) and 0.525 u (fp64).
TANH_ULPS = {np.float32: 2*1.465, np.float64: 2*0.525}


def _torch_dtype(hm):
  return torch.float32 if hm.dtype == np.float32 else torch.float64


def _noise(nsteps, nenv, nu, dtype, seed, scale=1.0, uniform=False):
  gen = torch.Generator(device='cuda')
  gen.manual_seed(seed)
  if uniform:       # U(-1, 1): an open-loop action sequence
    return torch.rand(nsteps, nenv, nu, device='cuda', dtype=dtype, generator=gen)*2 - 1
  return scale*torch.randn(nsteps, nenv, nu, device='cuda', dtype=dtype, generator=gen)


def _start(name, precision, nenv, seed=4):
  """A rollout code object and a batch at seeded initial states, outputs current."""
  model = helpers.load_model(name)
  hm = W.HipModel(build.build_model(model, helpers.TASKS[name], precision, rollout=True))
  assert hm.rollout_caps & W.ROLLOUT_OUTPUTS and hm.rollout_caps & W.ROLLOUT_POLICY
  assert hm.rollout_caps >> W.ROLLOUT_WIDTH_SHIFT == 64
  hb = W.HipBatch(hm, nenv)
  qpos, qvel = helpers.initial_states(model, name, nenv, seed=seed)
  hb.set_state(qpos.T, qvel.T)
  hb.forward()
  return model, hm, hb


def _upload(policy, hm):
  return torch.from_numpy(policy.packed(hm.dtype)).cuda()


def _rollout(name, precision, nenv, nsteps, nsub=1, ctrl=None, policy=None, calls=None,
             seed=4):
  """All fields and the three trajectories after `nsteps` control steps issued as
  the calls of `calls` (lengths; default one call), plus the observation before."""
  _, hm, hb = _start(name, precision, nenv, seed)
  info, dt = hm.info, _torch_dtype(hm)
  nu, nobs = info.nu, info.nobs
  out = {'obs_out': torch.full((nsteps, nenv, nobs), -7.0, device='cuda', dtype=dt),
         'reward_out': torch.full((nsteps, nenv), -7.0, device='cuda', dtype=dt),
         'action_out': torch.full((nsteps, nenv, nu), -7.0, device='cuda', dtype=dt)}
  weights = None if policy is None else _upload(policy, hm)
  first = hb.read(W.FIELD_OBS)
  torch.cuda.synchronize()
  es, t = out['obs_out'].element_size(), 0
  for n in calls or [nsteps]:
    hb.rollout(
        n, nsub,
        ctrl=None if ctrl is None else (ctrl.data_ptr() + t*nenv*nu*es, 1, nu, nenv*nu),
        policy=None if policy is None else (weights.data_ptr(), policy.widths),
        reward_out=(out['reward_out'].data_ptr() + t*nenv*es, nenv),
        obs_out=(out['obs_out'].data_ptr() + t*nenv*nobs*es, nenv*nobs),
        action_out=(out['action_out'].data_ptr() + t*nenv*nu*es, nenv*nu))
    t += n
  assert t == nsteps
  res = {field: hb.read(fid) for field, fid in FIELDS}      # (synchronises)
  res.update((k, v.cpu().numpy()) for k, v in out.items())
  res['first_obs'] = first
  hb.free()
  hm.free()
  return res


def _assert_same(a, b, skip=()):
  for field in [f for f, _ in FIELDS] + list(TRAJECTORIES):
    if field not in skip:
      np.testing.assert_array_equal(a[field], b[field], err_msg=field)


# -- (a) per-step outputs equal single steps ---------------------------------------

@pytest.mark.parametrize('name,nenv,nsub,nsteps', [('cheetah', 130, 1, 5), ('hopper', 70, 4, 3)])
def test_per_step_outputs_equal_single_steps(name, nenv, nsub, nsteps):
  """Open loop.  cheetah: two workgroups and a 2-env tail; hopper: substeps, touch
  sensors in the observation."""
  _, hm, twin = _start(name, 'f32', nenv)
  nu = hm.info.nu
  acts = _noise(nsteps, nenv, nu, torch.float32, 0, uniform=True)
  got = _rollout(name, 'f32', nenv, nsteps, nsub, ctrl=acts)
  for t in range(nsteps):
    twin.step_device(acts[t].data_ptr(), 1, nu, nsub)
    np.testing.assert_array_equal(got['obs_out'][t], twin.read(W.FIELD_OBS), err_msg='obs %d' % t)
    np.testing.assert_array_equal(got['reward_out'][t], twin.read(W.FIELD_REWARD),
                                  err_msg='reward %d' % t)
  np.testing.assert_array_equal(got['action_out'], acts.cpu().numpy())
  for field, fid in FIELDS:
    np.testing.assert_array_equal(got[field], twin.read(fid), err_msg=field)
  assert got['stats'][0].max() > 0          # (contacts: the solver ran)
  twin.free()
  hm.free()


def test_null_outputs_are_skipped():
  """Rewards only (what ES wants): the other stores are skipped, the rest is the same."""
  _, hm, hb = _start('cheetah', 'f32', 130)
  acts = _noise(5, 130, 6, torch.float32, 0, uniform=True)
  rew = torch.full((5, 130), -7.0, device='cuda')
  hb.rollout(5, 1, ctrl=(acts.data_ptr(), 1, 6, 130*6), reward_out=(rew.data_ptr(), 130))
  full = _rollout('cheetah', 'f32', 130, 5, 1, ctrl=acts)
  for field, fid in FIELDS:
    np.testing.assert_array_equal(hb.read(fid), full[field], err_msg=field)
  np.testing.assert_array_equal(rew.cpu().numpy(), full['reward_out'])
  hb.free()
  hm.free()


# -- (b) one launch equals T launches ----------------------------------------------

@pytest.mark.parametrize('name,precision,nenv,nsteps', [
    ('cheetah', 'f32', 130, 5), ('cartpole', 'f64', 66, 70), ('cheetah', 'mixed', 66, 70)])
def test_one_launch_equals_single_launches(name, precision, nenv, nsteps):
  """Policy and noise; 70 steps are two chunks (64 + 6) inside one call."""
  model = helpers.load_model(name)
  dt = torch.float64 if precision == 'f64' else torch.float32
  nobs = {'cheetah': 17, 'cartpole': 5}[name]
  policy = rollout_cases.make_policy(nobs, (5, 64), model.nu, seed=1)
  noise = _noise(nsteps, nenv, model.nu, dt, 2, scale=0.3)
  kw = dict(ctrl=noise, policy=policy)
  one = _rollout(name, precision, nenv, nsteps, **kw)
  each = _rollout(name, precision, nenv, nsteps, calls=[1]*nsteps, **kw)
  _assert_same(one, each)
  if nsteps > 64:
    _assert_same(one, _rollout(name, precision, nenv, nsteps, calls=[64, nsteps - 64], **kw))
  assert not one['warn'].any()
  assert np.abs(one['action_out'] - noise.cpu().numpy()).max() > 0.05     # (the policy acted)


# -- (c) replay identity -----------------------------------------------------------

def test_recorded_actions_replay_the_rollout():
  policy = rollout_cases.make_policy(17, (5, 64), 6, seed=3)
  noise = _noise(5, 130, 6, torch.float32, 4, scale=0.3)
  closed = _rollout('cheetah', 'f32', 130, 5, ctrl=noise, policy=policy)
  replay = _rollout('cheetah', 'f32', 130, 5, ctrl=torch.from_numpy(closed['action_out']).cuda())
  _assert_same(closed, replay)
  assert closed['stats'][0].max() > 0


# -- (d) the policy computes the MLP -----------------------------------------------

@pytest.mark.parametrize('name,precision', [('cheetah', 'f32'), ('cartpole', 'f64')])
@pytest.mark.parametrize('hidden', [(3,), (64,), (3, 64), (64, 3)])
def test_the_policy_computes_the_mlp(name, precision, hidden):
  """action_out[t] - noise[t] against the fp64 model on o_t (o_0: the observation
  before the call, o_t = obs_out[t-1]) within twice its forward error bound."""
  case = rollout_cases.policy_case(name, precision, hidden)
  real = np.float32 if precision == 'f32' else np.float64
  noise = _noise(case['nsteps'], case['nenv'], case['nu'],
                 torch.float32 if precision == 'f32' else torch.float64, 5, scale=0.1)
  got = _rollout(name, precision, case['nenv'], case['nsteps'], ctrl=noise, policy=case['policy'])
  obs = np.concatenate([got['first_obs'][None], got['obs_out'][:-1]]).astype(np.float64)
  want, bound = case['policy'].forward(obs, real, TANH_ULPS[real])
  err = np.abs(got['action_out'].astype(np.float64) - noise.cpu().numpy().astype(np.float64) - want)
  print('policy error / bound: max %.3f' % (err/bound).max())
  assert np.all(err <= 2*bound), float((err/bound).max())
  assert np.abs(want).max() > 0.1 and not got['warn'].any()


# -- (e) bad actions ---------------------------------------------------------------

def test_nan_policy_output_warns_and_applies_zero_controls():
  policy = rollout_cases.make_policy(17, (5,), 6, seed=6)
  policy.biases[-1][:] = np.nan
  bad = _rollout('cheetah', 'f32', 130, 3, policy=policy)
  zero = _rollout('cheetah', 'f32', 130, 3, ctrl=torch.zeros(3, 130, 6, device='cuda'))
  assert np.all(bad['warn'] & 128)                  # DMC_WARN_BADCTRL
  assert not zero['warn'].any()
  assert np.isnan(bad['action_out']).all()
  _assert_same(bad, zero, skip=('warn', 'action_out'))


# -- (f) the rollout build is still the physics ------------------------------------

@pytest.mark.parametrize('name', ['cheetah', 'cartpole'])
def test_fp64_rollout_build_against_the_oracle(name):
  """Teacher-forced from oracle states like helpers._teacher_forced, every step a
  T = 1 rollout: relative error of qpos / qvel <= 1e-9 per step."""
  # pylint: disable=protected-access
  nenv, steps = 64, 10
  model, hm, hb = _start(name, 'f64', nenv, seed=7)
  qpos, qvel = helpers.initial_states(model, name, nenv, seed=7)
  _, datas = helpers._oracle_envs(model, qpos, qvel)
  rs = np.random.RandomState(11)
  errs = []
  for _ in range(steps):
    oq = np.array([d.qpos.copy() for d in datas])
    ov = np.array([d.qvel.copy() for d in datas])
    ow = np.array([d.qacc_warmstart.copy() for d in datas])
    skip = np.array([helpers._degenerate(d, model) for d in datas])
    hb.set_state(oq.T, ov.T, ow.T)
    ctrl = rs.uniform(-1, 1, (nenv, model.nu))
    dev = torch.from_numpy(ctrl).cuda()
    torch.cuda.synchronize()
    hb.rollout(1, 1, ctrl=(dev.data_ptr(), 1, model.nu, 0))
    q = hb.read(W.FIELD_QPOS).T.astype(np.float64)
    v = hb.read(W.FIELD_QVEL).T.astype(np.float64)
    for i, d in enumerate(datas):
      d.ctrl[:] = ctrl[i]
      skip[i] |= helpers._degenerate(d, model)
      d.physics_step()
    nq = np.array([d.qpos.copy() for d in datas])
    nv = np.array([d.qvel.copy() for d in datas])
    errs.append(np.maximum(helpers.rel_err(q, nq), helpers.rel_err(v, nv))[~skip])
  assert not hb.read(W.FIELD_WARN).any()
  e = np.concatenate(errs)
  print('%s fp64 rollout build: max per-step error %.3g' % (name, e.max()))
  assert e.size > steps*nenv//2 and e.max() <= 1e-9, e.max()
  hb.free()
  hm.free()


# -- (g) refusals ------------------------------------------------------------------

def _still_steps(hb, nu):
  t0 = hb.read(W.FIELD_TIME)
  hb.step_host(np.zeros((hb.nenv, nu)), 1)
  assert np.all(hb.read(W.FIELD_TIME) > t0)
  assert np.all(np.isfinite(hb.read(W.FIELD_QPOS)))


def test_refusals_leave_a_batch_that_steps():
  model = helpers.load_model('cheetah')
  acts = _noise(2, 70, 6, torch.float32, 8, uniform=True)
  ctrl = (acts.data_ptr(), 1, 6, 70*6)
  hm, hb = helpers._device_batch(model, helpers.TASKS['cheetah'], 'f32', 70)   # pylint: disable=protected-access
  assert hm.rollout_caps == 0
  with pytest.raises(W.Error, match='rollout=True'):
    hb.rollout(2, 1, ctrl=ctrl)
  _still_steps(hb, 6)
  hb.free()
  hm.free()

  _, hm, hb = _start('cheetah', 'f32', 70)
  weights = torch.zeros(70*70 + 4096, device='cuda')       # (room for every shape below)
  for widths, message in (((65, 6), '65 units'), ((3, 3, 3, 6), '1 or 2 hidden layers'),
                          ((3,), '1 or 2 hidden layers'), ((3, 7), '7 values')):
    with pytest.raises(W.Error, match=message):
      hb.rollout(2, 1, policy=(weights.data_ptr(), widths))
    _still_steps(hb, 6)
  hb.set_masked(True)
  with pytest.raises(W.Error, match='env mask'):
    hb.rollout(2, 1, ctrl=ctrl)
  hb.set_masked(False)
  _still_steps(hb, 6)
  hb.episodes_enable(10)
  with pytest.raises(W.Error, match='per-env episodes'):
    hb.rollout(2, 1, ctrl=ctrl)
  _still_steps(hb, 6)
  assert hb.episode_read(W.EPISODE_STEP).tolist() == [1]*70
  hb.free()
  hm.free()


def test_timer_counts_control_steps():
  _, hm, hb = _start('cheetah', 'f32', 130)
  acts = _noise(5, 130, 6, torch.float32, 7, uniform=True)
  hb.timer_start()
  hb.rollout(5, 1, ctrl=(acts.data_ptr(), 1, 6, 130*6))
  ms, count = hb.timer_stop()
  assert count == 5 and ms > 0
  hb.free()
  hm.free()


# -- (h) VecEnv.rollout ------------------------------------------------------------

def _vec_env(**kw):
  from dm_control_amd import vec_env
  # time limit 0.065 s: the episode ends with the 7th step of 0.01 s
  return vec_env.VecEnv('cheetah', 'run', 130, seed=0, torch_io=True,
                        task_kwargs={'time_limit': 0.065}, **kw)


def test_vec_env_rollout():
  from dm_control_amd import vec_env
  with pytest.raises(ValueError, match='torch_io'):
    vec_env.VecEnv('cheetah', 'run', 4, rollout=True)
  with pytest.raises(ValueError, match='lock-step'):
    vec_env.VecEnv('cheetah', 'run', 4, torch_io=True, per_env_episodes=True, rollout=True)
  policy = rollout_cases.make_policy(17, (64, 64), 6, seed=9)
  noise = _noise(10, 130, 6, torch.float32, 10, scale=0.2)
  env, twin = _vec_env(rollout=True), _vec_env(rollout=True)
  assert 'one env per lane' in env.environment.physics.kernel_shape
  first = env.reset()
  np.testing.assert_array_equal(first.cpu().numpy(), twin.reset().cpu().numpy())
  out = env.rollout(10, policy=policy, noise=noise)
  assert out['obs'].shape == (7, 130, 17) and out['actions'].shape == (7, 130, 6)
  assert out['rewards'].shape == (7, 130) and out['dones'].shape == (7, 130)
  assert out['dones'][-1].all() and not out['dones'][:-1].any()
  np.testing.assert_array_equal(out['terminal_observation'].cpu().numpy(),
                                out['obs'][-1].cpu().numpy())
  want = policy.forward(first.cpu().numpy().astype(np.float64)) + noise[0].cpu().numpy()
  np.testing.assert_allclose(out['actions'][0].cpu().numpy(), want, rtol=0, atol=1e-4)
  # the same seven steps through VecEnv.step, fed the recorded actions
  for t in range(7):
    obs, rew, dones, infos = twin.step(out['actions'][t])
    np.testing.assert_array_equal(rew.cpu().numpy(), out['rewards'][t].cpu().numpy())
    np.testing.assert_array_equal(dones.cpu().numpy(), out['dones'][t].cpu().numpy())
    if t < 6:
      np.testing.assert_array_equal(obs.cpu().numpy(), out['obs'][t].cpu().numpy())
  np.testing.assert_array_equal(infos['terminal_observation'].cpu().numpy(),
                                out['obs'][6].cpu().numpy())
  np.testing.assert_array_equal(obs.cpu().numpy(), out['next_obs'].cpu().numpy())
  # the observation after a reset, and a second call starts the new episode
  assert not np.array_equal(out['next_obs'].cpu().numpy(), out['obs'][-1].cpu().numpy())
  again = env.rollout(3, actions=noise[:3])
  assert again['obs'].shape[0] == 3 and not again['dones'].any()
  assert 'terminal_observation' not in again
  for t in range(3):
    obs, rew, _, _ = twin.step(noise[t])
    np.testing.assert_array_equal(obs.cpu().numpy(), again['obs'][t].cpu().numpy())
    np.testing.assert_array_equal(rew.cpu().numpy(), again['rewards'][t].cpu().numpy())
  np.testing.assert_array_equal(again['next_obs'].cpu().numpy(), again['obs'][-1].cpu().numpy())
  with pytest.raises(ValueError, match='rollout=True'):
    plain = _vec_env()
    plain.rollout(3, actions=noise[:3])
  plain.close()
  env.close()
  twin.close()
