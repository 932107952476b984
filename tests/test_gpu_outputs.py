"""What the step hands back -- observation, reward, sensordata, exported frames --
of every kernel shape the product can select, against the fp64 host model of
the output stage (tests/output_model.py, pinned to the oracle and the goldens on
the CPU by tests/test_output_model.py).

The model is evaluated at the device's own read-back state, so dynamics error
never enters a bound: only the output stage is compared.

  * observe path: the case states of tests/output_cases.py (every reachable
    branch of every `tolerance()` term), `forward()`;
  * step path: one control step from 129 plausible states, outputs compared at
    the post-step state.
One case per distinct (domain, precision, mode, group) of the selection matrix
(the first line of each), plus the 8 / 16 lanes-per-env builds at 61 envs.
Every variant of the domain's tasks (sparse, move speeds, target sizes) runs on
the same batch through `set_task_params`.

Bounds (output_model.py): fp64 1e-9 in `helpers.rel_err` form per output
class; fp32 / mixed 4x the CPU figure of the class in eps32*scale; copies of
the state bit-identical.  A reward sample is left out only when a margin-0
term's input lies within its own tolerance of a bound, at most 1 % of a case.

The one-lane kernel's second observation layout (explicit strides instead of
the LDS transpose) cannot be selected through the runtime, which always hands
the kernel the agent layout; the two stores are compared bit for bit on the
host (tests/test_kernel_sanitizers.py, observe mode of the shim).
"""

import os

import numpy as np
import pytest

import helpers
import output_cases as cases
import output_model as M
import selection_matrix as sm
from dm_control_amd import build
from dm_control_amd import wrapper
from test_gpu_selection import NSUB

pytestmark = pytest.mark.gpu

W = wrapper


def _first_lines():
  seen, out = set(), []
  for line in sm.SHIPPED:
    key = line[:4]
    if key in seen or line[2] == sm.REFUSED:     # (the humanoid's `mixed` refusal:
      continue                                   # pinned by tests/test_gpu_selection.py)
    seen.add(key)
    out.append(line)
  return out


LINES = _first_lines()
SMALL = [g for g in sm.SMALL_GROUPS if g not in sm.SMALL_GROUPS_REFUSED]
SMALL_NENV = 61


def _read_state(hb):
  return {name: hb.read(getattr(W, 'FIELD_' + name.upper())).T.astype(np.float64)
          for name in ('qpos', 'qvel', 'ctrl')}


def _compare(hb, model, domain, variant, precision, what):
  """The outputs the batch holds against the model at the state it holds.
  -> {class: largest error in the class's unit}."""
  label, _, param_i, param_r = variant
  info = hb.model.info
  s = _read_state(hb)
  taskdata = (hb.read(W.FIELD_TASKDATA).T.astype(np.float64) if info.ntaskdata > 0
              else None)
  want = M.evaluate(model, helpers.TASKS[domain], param_i, param_r, s['qpos'], s['qvel'],
                    s['ctrl'], taskdata)
  n = len(want.reward)
  got = M.Outputs()
  got.obs = hb.read(W.FIELD_OBS).astype(np.float64)
  got.reward = hb.read(W.FIELD_REWARD).astype(np.float64)
  got.sensordata = hb.read(W.FIELD_SENSORDATA).T.astype(np.float64)
  got.xpos = hb.read(W.FIELD_XPOS).T.astype(np.float64).reshape(n, -1, 3)
  got.xmat = hb.read(W.FIELD_XMAT).T.astype(np.float64).reshape(n, -1, 9)
  assert not hb.read(W.FIELD_WARN).any()
  assert got.obs.shape == want.obs.shape

  # touch: not modelled; the observation is log1p of the sensor the device stored
  touch_obs = np.array(want.obs_kinds) == 'touch'
  touch_sens = np.array(want.sensor_kinds) == 'touch'
  if touch_obs.any():
    assert touch_obs.sum() == touch_sens.sum()
    eps = np.finfo(hb.model.dtype).eps
    np.testing.assert_allclose(got.obs[:, touch_obs], np.log1p(got.sensordata[:, touch_sens]),
                               rtol=8*eps, atol=8*eps)
    assert (got.sensordata[:, touch_sens] >= 0).all()

  pairs = {
      'pos': [('xpos', got.xpos.reshape(n, -1), want.xpos.reshape(n, -1))],
      'rot': [('xmat', got.xmat.reshape(n, -1), want.xmat.reshape(n, -1))],
      'vel': [], 'state': [],
      'reward': [('reward', got.reward.reshape(n, 1), want.reward.reshape(n, 1))]}
  for name, g, w, kinds in (('obs', got.obs, want.obs, want.obs_kinds),
                            ('sensordata', got.sensordata, want.sensordata,
                             want.sensor_kinds)):
    kinds = np.array(kinds)
    for kind in pairs:
      if (kinds == kind).any():
        pairs[kind].append(('%s.%s' % (name, kind), g[:, kinds == kind], w[:, kinds == kind]))
  real = hb.model.dtype
  for name, g, w in pairs['state']:     # copies of qpos / qvel: the stored words
    np.testing.assert_array_equal(g, w.astype(real).astype(np.float64), err_msg=name)

  scale = M.scales(want)
  if precision == 'f64':
    tol = {k: 1e-9*scale[k] for k in M.CLASSES + ('state',)}
  else:
    tol = M.fp32_tolerances(want)
  left_out = M.excluded(want, tol)
  assert left_out.sum() <= cases.MAX_EXCLUDED*n, (left_out.sum(), n)
  figure = {}
  for kind in M.CLASSES:
    keep = ~left_out if kind == 'reward' else np.ones(n, bool)
    for name, g, w in pairs[kind]:
      if precision == 'f64':
        err = helpers.rel_err(g, w)[keep]
        figure[kind] = max(figure.get(kind, 0.0), float(err.max()))
        assert err.max() <= 1e-9, (what, label, name, err.max())
      else:
        err = (np.abs(g - w).max(axis=1)/(M.EPS32*scale[kind]))[keep]
        figure[kind] = max(figure.get(kind, 0.0), float(err.max()))
        assert err.max() <= M.bound_in_eps(kind), (
            what, label, name, 'env %d: %.1f eps32*scale, bound %.1f'
            % (np.nonzero(keep)[0][err.argmax()], err.max(), M.bound_in_eps(kind)))
  print('OBSERVED outputs %s %s: %s, left out %d of %d' % (
      what, label, ' '.join('%s %.2e' % (k, v) for k, v in sorted(figure.items())),
      left_out.sum(), n) + ('' if precision == 'f64' else ' (eps32*scale)'))
  return figure


def _run_case(domain, nenv, what, **build_kwargs):
  precision = build_kwargs['precision']
  assert os.environ.get('DMC_ALLOW_OVERBUDGET') != '1'
  model, qpos, qvel, ctrl, taskdata = cases.states(domain)
  hm = W.HipModel(build.build_model(model, helpers.TASKS[domain], **build_kwargs))
  hb = W.HipBatch(hm, nenv)
  hb.set_aux_outputs(True)
  variants = [v for v in cases.VARIANTS[domain] if v[1] is None]
  # designed states last: a smaller batch keeps them (and the partial last block)
  pick = np.arange(cases.NENV)[-nenv:]
  more_q, more_v = helpers.initial_states(model, domain, cases.NENV - cases.NFIRST,
                                          seed=cases.SEED + 2)
  step_q = np.vstack([qpos[:cases.NFIRST], more_q])[pick]
  step_v = np.vstack([qvel[:cases.NFIRST], more_v])[pick]
  zeros = np.zeros((max(model.nv, 1), nenv))
  for variant in variants:
    hb.set_task_params(variant[2], variant[3])
    if taskdata is not None:
      hb.write(W.FIELD_TASKDATA, taskdata[pick].T)
    # observe path
    hb.set_state(qpos[pick].T, qvel[pick].T, zeros, np.zeros(nenv))
    hb.write(W.FIELD_CTRL, ctrl[pick].T)
    hb.forward()
    _compare(hb, model, domain, variant, precision, what + ' observe')
    # step path
    hb.set_state(step_q.T, step_v.T, zeros, np.zeros(nenv))
    hb.step_host(ctrl[pick], NSUB[domain])
    _compare(hb, model, domain, variant, precision, what + ' step')
  hb.free()
  hm.free()


@pytest.mark.parametrize('line', LINES, ids=sm.line_id)
def test_outputs_match_host_model(line):
  _run_case(line[0], cases.NENV, sm.line_id(line), **sm.build_args(line))


@pytest.mark.parametrize('domain,group,precision', SMALL)
def test_outputs_of_eight_and_sixteen_lanes_per_env(domain, group, precision):
  _run_case(domain, SMALL_NENV,
            '%s-%s-g%d x%d' % (domain, precision, group, SMALL_NENV),
            precision=precision, mode='coop', group=group)


def test_the_case_list_is_the_selection_matrix():
  assert len(LINES) == 39 and len(SMALL) == 11
  assert {line[0] for line in LINES} == set(cases.DOMAINS)
