"""States for the output-stage tests: per domain 129 envs (two wavefronts and
one lane, as `PARITY_NENV` of test_gpu_selection.py) under a fixed seed.

The first 64 are `helpers.initial_states`.  The other 65 are designed so that
every reachable branch of every `tolerance()` term of the reward is evaluated
(the observe path runs no integrator, so any finite state will do): root
velocities on both sides of every speed bound and cut-off, root heights and
orientations on both sides of the standing / upright bounds, poles inside and
outside their cones, tips and fingers solved onto both sides of their target
radii, and `ctrl` rows of exactly 0 and +-1 next to uniform ones.

VARIANTS lists, per domain, the (label, poles, task_param_i, task_param_r) of
every shipped task whose outputs differ.  tests/test_output_model.py asserts
that every reachable (term, branch) pair of every variant is hit by at least
MIN_HITS envs and that no reward sample lies within its input's tolerance of a
margin-0 bound.
"""

import numpy as np

import helpers
import output_model
from dm_control_amd import codegen

NENV, NFIRST, SEED = 129, 64, 20271
MIN_HITS = 4
MAX_EXCLUDED = 0.01      # as in tests/test_gpu_selection.py

# domain -> ((label, poles or None, task_param_i, task_param_r), ...)
VARIANTS = {
    'cartpole': (('smooth', None, 0, ()), ('sparse', None, 1, ()),
                 ('two_poles', 2, 2, ()), ('three_poles', 3, 2, ())),
    'cheetah': (('run', None, 0, ()),),
    'humanoid': (('stand', None, 0, (0.0,)), ('walk', None, 0, (1.0,)),
                 ('run', None, 0, (10.0,))),
    'walker': (('stand', None, 0, (0.0,)), ('walk', None, 0, (1.0,)),
               ('run', None, 0, (8.0,))),
    'pendulum': (('swingup', None, 0, ()),),
    'acrobot': (('swingup', None, 0, ()), ('swingup_sparse', None, 1, ())),
    'hopper': (('stand', None, 0, ()), ('hop', None, 1, ())),
    'reacher': (('easy', None, 0, (0.05 + 0.01,)), ('hard', None, 0, (0.015 + 0.01,))),
    'point_mass': (('easy', None, 0, ()),),
}
DOMAINS = tuple(VARIANTS)

# (term, branch) pairs that no state reaches: none.  The pairs that look out of
# reach are reached exactly: a quadratic `small_control` term is in bounds at
# ctrl == 0 and on the floor at |ctrl| == 1 (the constant ctrl rows); the
# humanoid's `move` is on the floor and its `dont_move` in bounds at a CoM
# velocity of exactly 0 (the envs at rest); its `upright` is on the floor at
# torso_upright == -1 (the root quaternions that turn it upside down exactly).
UNREACHABLE = ()


def model_of(domain, poles=None):
  import device_init_model
  return device_init_model.case_model(domain, poles)


def _dof(model, joint):
  j = model.names['joint'].index(joint)
  return int(model.jnt_qposadr[j]), int(model.jnt_dofadr[j])


def _cycle(values, n, rs):
  out = np.resize(np.asarray(values, np.float64), n)
  rs.shuffle(out)
  return out


def _acrobot_solve(model, want_xz):
  """Joint angles [n, 2] that put the tip at want_xz [n, 2] (x, z): Newton on
  the host model's kinematics from a bent start."""
  site = codegen.task_sites(model, codegen.TASK_ACROBOT)[0]

  def tip(q):
    f = output_model.kinematics(model, q, np.zeros_like(q))
    p = output_model._site(model, f, site)      # pylint: disable=protected-access
    return p[:, [0, 2]]
  q = np.tile([0.3, -0.6], (len(want_xz), 1))
  q[::2] *= -1
  for _ in range(60):
    r = tip(q) - want_xz
    h = 1e-6
    jac = np.stack([(tip(q + h*np.eye(2)[k]) - tip(q - h*np.eye(2)[k]))/(2*h)
                    for k in range(2)], axis=2)
    step = np.linalg.solve(jac, r[:, :, None])[:, :, 0]
    q -= np.clip(step, -0.3, 0.3)
  assert np.abs(tip(q) - want_xz).max() < 1e-9
  return q


def states(domain, poles=None):
  """-> model, qpos [129, nq], qvel [129, nv], ctrl [129, nu], taskdata
  [129, ntaskdata] or None."""
  model = model_of(domain, poles)
  task = helpers.TASKS[domain]
  rs = np.random.RandomState(SEED)
  n, k = NENV, NENV - NFIRST
  q0, v0 = helpers.initial_states(model, domain, NFIRST, seed=SEED)
  q1, v1 = helpers.initial_states(model, domain, k, seed=SEED + 1)
  ntd = codegen.task_data_size(task)
  taskdata = None
  if domain in ('cheetah', 'walker', 'hopper'):
    _, vx = _dof(model, 'rootx')
    top = {'cheetah': 10.0, 'walker': 8.0, 'hopper': 2.0}[domain]
    v1[:, vx] += _cycle([-3, -1, -0.3, 0.15, 0.3, 0.45, 0.6, 0.75, 0.9, 1.3, 0.5*top,
                         0.8*top, 0.95*top, 1.1*top, 1.5*top, 2.5*top], k, rs)
    qz, _ = _dof(model, 'rootz')
    if domain == 'walker':
      q1[:, qz] = rs.uniform(-0.6, 0.3, k)
    if domain == 'hopper':     # from folded (low) to stretched (height > 0.6)
      lim = model.jnt_limited.astype(bool)
      lo, hi = model.jnt_range[lim].T
      fold = np.linspace(0.0, 1.0, k)[:, None]
      q1[:, lim] = fold*rs.uniform(lo, hi, (k, lim.sum()))
  elif domain == 'humanoid':
    q1[:, 2] = rs.uniform(0.4, 1.9, k)
    tilt = _cycle(np.linspace(0, np.pi, 16), k, rs)
    axis = rs.randn(k, 3)*[1, 1, 0.2]
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    q1[:, 3:7] = np.hstack([np.cos(tilt/2)[:, None], axis*np.sin(tilt/2)[:, None]])
    v1[:, 0:3] += rs.randn(k, 3)*_cycle([0.3, 0.6, 1.5, 4, 7, 9, 11, 14], k, rs)[:, None]
    # upside down exactly (torso_upright -1: the linear term's cut-off)
    for i, quat in enumerate(([0, 1, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, -1, 0],
                              [0, 0.6, 0.8, 0])):
      q1[i, 3:7] = quat
      q1[i, 7:] = model.qpos0[7:]
    # at rest (CoM velocity exactly 0: `dont_move` in bounds, `move` on the floor)
    v1[5:11] = 0
  elif domain == 'cartpole':
    q1[:, 0] = _cycle([0, -0.2, 0.1, 0.24, -0.26, 0.3, -0.9, 1.5, 0, 0.05], k, rs)
    for p in range(1, model.nq):
      q1[:, p] = _cycle([0.01, 0.03, -0.08, 0.09, -0.11, 0.12, 0.5, -2.0, 3.1], k, rs)
    # poles of the multi-pole layouts hang off each other: keep some chains upright
    # (not within rounding of cos = 1, the upper bound of the sparse reward's cone)
    q1[::3, 2:] = rs.uniform(0.005, 0.03, (len(q1[::3]), model.nq - 2))*rs.choice(
        [-1, 1], (len(q1[::3]), model.nq - 2))
    v1[:] = rs.randn(k, model.nv)*_cycle([0.5, 2, 4, 6, 9], k, rs)[:, None]
    v1[::7] = 0
  elif domain == 'pendulum':
    q1[:, 0] = _cycle([0.01, 0.05, -0.1, 0.13, -0.135, 0.145, -0.15, 0.3, 1.5, 3.1], k, rs)
  elif domain == 'acrobot':
    radius = _cycle([0.02, 0.08, 0.15, 0.19, 0.21, 0.25, 0.4, 0.9], k, rs)
    phi = rs.uniform(-1.0, 1.0, k)
    target = np.array([0.0, 4.0])
    q1[:] = _acrobot_solve(model, target + radius[:, None]*np.stack(
        [np.sin(phi), -np.cos(phi)], axis=1))
  elif domain == 'point_mass':
    r = _cycle([0, 0, 0.004, 0.01, 0.014, 0.016, 0.02, 0.028, 0.05, 0.1, 0.25], k, rs)
    phi = rs.uniform(-np.pi, np.pi, k)
    q1[:] = r[:, None]*np.stack([np.cos(phi), np.sin(phi)], axis=1)
  qpos, qvel = np.vstack([q0, q1]), np.vstack([v0, v1])
  if domain == 'reacher':
    # targets around the finger, on both sides of both radii (0.025 and 0.06)
    f = output_model.kinematics(model, qpos, qvel)
    finger = output_model._site(                      # pylint: disable=protected-access
        model, f, codegen.task_sites(model, task)[0])[:, :2]
    r = np.concatenate([rs.uniform(0.0, 0.3, NFIRST), _cycle(
        [0.003, 0.012, 0.02, 0.024, 0.026, 0.03, 0.045, 0.058, 0.062, 0.08, 0.15], k, rs)])
    phi = rs.uniform(-np.pi, np.pi, n)
    taskdata = finger + r[:, None]*np.stack([np.cos(phi), np.sin(phi)], axis=1)
  elif ntd:
    taskdata = np.tile(codegen.task_data_default(model, task), (n, 1))
  ctrl = rs.uniform(-1, 1, (n, model.nu))
  ctrl[NFIRST + 12:NFIRST + 17] = 0
  ctrl[NFIRST + 17:NFIRST + 22] = 1
  ctrl[NFIRST + 22:NFIRST + 27] = -1
  return model, qpos, qvel, ctrl, taskdata


def reachable(out):
  """{(term, branch)} that states of a variant can reach."""
  return {(t.name, b) for t in out.terms for b in t.reach} - set(UNREACHABLE)


def coverage(out):
  """{(term, branch): number of envs}."""
  hits = {}
  for t in out.terms:
    for b in np.unique(t.branch):
      hits[(t.name, int(b))] = int((t.branch == b).sum())
  return hits
