"""Host model of the device's output stage (numpy; no GPU, no oracle).

`evaluate` restates, for a batch of states, what `observe_stage`,
`task_outputs` and `write_outputs` of csrc/dmc_kernels.hip (and their
counterparts in csrc/dmc_coop.hip) hand over: body frames, subtree centres of
mass and their velocities, the non-touch sensors, the flat observation in the
kernel's order and the reward, plus the input and the branch of every
`tolerance()` term of the reward.

Nothing here is taken from the kernel.  The kinematics follow the joint chain
from the model tables; body velocities are the joint-Jacobian sums
  v(p) = sum over the dofs d on the path to the body of J_d(p) qvel_d
(slide: axis; hinge: axis x (p - anchor); free / ball rotation: the local
angular velocity turned into the world frame), which is not the spatial-
velocity recursion of the kernels and the oracle.  The reward comes from
tests/task_formulas.py (validated by tests/golden/tasks.json).
tests/test_output_model.py pins the model to the oracle at 1e-12.

Every arithmetic step honours `dtype`: the same code run in float32 is the
independent fp32 reference that the fp32 / mixed bounds come from.

Tolerances (device vs the model evaluated at the device's own read-back state)
------------------------------------------------------------------------------
fp64: the project's 1e-9 in `helpers.rel_err` form, per output class.
fp32 / mixed: BOUND_IN_EPS[class] * eps32 * scale, where scale is a fixed rule
computed from the float64 model alone (`scales`):
  pos     max(1, largest |xpos| component of the env): xpos, xipos,
          subtree_com, and every observation entry / sensor that is a position
          or a difference of positions
  rot     1: xmat entries and the observation entries copied from them
  vel     max(1, largest body speed of the env with every joint's share taken
          in magnitude): max over bodies i of sum_d |J_d(xipos_i)| |qvel_d|.
          This is the body's speed bound without cancellation; a hinge's or a
          free joint's share is |omega| times its lever, so it contains
          |omega| * extent.  subtree_linvel and what is copied from it
  reward  1
  state   0: observation entries and sensors that are copies of qpos / qvel
          (bit-identical to the read-back state)
CPU_FIGURE[class] is the largest error of this model run in float32 against
the float64 run over all states of tests/output_cases.py, in units of
eps32 * scale (tests/test_output_model.py recomputes it and fails if it drifts
by more than a factor of 2).  The device bound is 4x that figure: the device
contracts multiply-adds and divides by reciprocal, an independent float32
evaluation does neither (the margin tests/device_init_model.py gives its
bounds for the same reason).
"""

import collections

import numpy as np

import task_formulas
from dm_control_amd import codegen
from dm_control_amd.mjcf import model as mdl

CLASSES = ('pos', 'rot', 'vel', 'reward')
# measured by tests/test_output_model.py::test_fp32_figures (units: eps32*scale)
CPU_FIGURE = {'pos': 3.8, 'rot': 3.5, 'vel': 2.2, 'reward': 2.3}
EPS32 = float(np.finfo(np.float32).eps)


def bound_in_eps(kind):
  return 4.0*CPU_FIGURE[kind]


# ---------------------------------------------------------------------------
# quaternions (w, x, y, z), batched on the leading axis
# ---------------------------------------------------------------------------
def _qmul(a, b):
  aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
  bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
  return np.stack([aw*bw - ax*bx - ay*by - az*bz,
                   aw*bx + ax*bw + ay*bz - az*by,
                   aw*by - ax*bz + ay*bw + az*bx,
                   aw*bz + ax*by - ay*bx + az*bw], axis=-1)


def _qnorm(q):
  return q/np.sqrt(np.sum(q*q, axis=-1, keepdims=True))


def _qmat(q):
  w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
  rows = [w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y),
          2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),
          2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z]
  return np.stack(rows, axis=-1).reshape(q.shape[:-1] + (3, 3))


def _rot(mat, v):
  """mat [B, 3, 3] applied to v [3] or [B, 3]."""
  v = np.broadcast_to(v, mat.shape[:-2] + (3,))
  return np.sum(mat*v[..., None, :], axis=-1)


def _cross(a, b):
  return np.stack([a[..., 1]*b[..., 2] - a[..., 2]*b[..., 1],
                   a[..., 2]*b[..., 0] - a[..., 0]*b[..., 2],
                   a[..., 0]*b[..., 1] - a[..., 1]*b[..., 0]], axis=-1)


# ---------------------------------------------------------------------------
# kinematics and velocities
# ---------------------------------------------------------------------------
class Frames:
  """xpos [B, nbody, 3], xmat [B, nbody, 9], xipos, subtree_com,
  subtree_linvel [B, nbody, 3], body_speed_bound [B] (fp: the `vel` scale)."""


def kinematics(m, qpos, qvel, dtype=np.float64):
  dt = np.dtype(dtype).type
  c = lambda a: np.asarray(a, np.float64).astype(dt)
  qpos, qvel = c(qpos), c(qvel)
  nb, bsz = int(m.nbody), len(qpos)
  body_pos, body_quat = c(m.body_pos).reshape(nb, 3), c(m.body_quat).reshape(nb, 4)
  body_ipos, body_mass = c(m.body_ipos).reshape(nb, 3), c(m.body_mass)
  jnt_pos, jnt_axis = c(m.jnt_pos).reshape(-1, 3), c(m.jnt_axis).reshape(-1, 3)
  qpos0 = c(m.qpos0)
  xpos = np.zeros((bsz, nb, 3), dt)
  xquat = np.zeros((bsz, nb, 4), dt)
  xquat[..., 0] = 1
  xmat = np.zeros((bsz, nb, 3, 3), dt)
  xmat[:, 0] = np.eye(3, dtype=dt)
  # per dof: how a unit of qvel moves a point p of a body below it
  #   ('lin', axis [B, 3]) or ('ang', axis [B, 3], anchor [B, 3])
  dof_motion = [None]*int(m.nv)
  for b in range(1, nb):
    par = int(m.body_parentid[b])
    pos = xpos[:, par] + _rot(xmat[:, par], body_pos[b])
    quat = _qmul(xquat[:, par], np.broadcast_to(body_quat[b], (bsz, 4)))
    for j in range(int(m.body_jntadr[b]), int(m.body_jntadr[b]) + int(m.body_jntnum[b])):
      kind, qa, da = int(m.jnt_type[j]), int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
      if kind == mdl.JNT_FREE:
        pos = qpos[:, qa:qa + 3].copy()
        quat = _qnorm(qpos[:, qa + 3:qa + 7])
        rot = _qmat(quat)
        for k in range(3):
          e = np.zeros((bsz, 3), dt)
          e[:, k] = 1
          dof_motion[da + k] = ('lin', e)
          dof_motion[da + 3 + k] = ('ang', rot[:, :, k], pos)
        continue
      rot = _qmat(quat)
      anchor = pos + _rot(rot, jnt_pos[j])
      axis = _rot(rot, jnt_axis[j])
      if kind == mdl.JNT_SLIDE:
        pos = pos + axis*(qpos[:, qa] - qpos0[qa])[:, None]
        dof_motion[da] = ('lin', axis)
        continue
      if kind == mdl.JNT_HINGE:
        half = (qpos[:, qa] - qpos0[qa])*dt(0.5)
        local = np.concatenate([np.cos(half)[:, None],
                                jnt_axis[j]*np.sin(half)[:, None]], axis=1)
        dof_motion[da] = ('ang', axis, anchor)
      else:   # ball
        local = _qnorm(qpos[:, qa:qa + 4])
      quat = _qmul(quat, local)
      pos = anchor - _rot(_qmat(quat), jnt_pos[j])
      if kind == mdl.JNT_BALL:
        rot = _qmat(quat)
        for k in range(3):
          dof_motion[da + k] = ('ang', rot[:, :, k], anchor)
    quat = _qnorm(quat)
    xpos[:, b], xquat[:, b], xmat[:, b] = pos, quat, _qmat(quat)
  xipos = xpos + np.sum(xmat*body_ipos[None, :, None, :], axis=-1)

  # the dofs on the path from the world to each body
  def chain(b):
    while b > 0 and int(m.body_dofnum[b]) == 0:
      b = int(m.body_parentid[b])
    if b == 0:
      return []
    d, out = int(m.body_dofadr[b]) + int(m.body_dofnum[b]) - 1, []
    while d >= 0:
      out.append(d)
      d = int(m.dof_parentid[d])
    return out[::-1]
  vel = np.zeros((bsz, nb, 3), dt)
  speed_bound = np.zeros((bsz, nb), np.float64)
  for b in range(1, nb):
    for d in chain(b):
      motion = dof_motion[d]
      col = motion[1] if motion[0] == 'lin' else _cross(motion[1], xipos[:, b] - motion[2])
      term = col*qvel[:, d:d + 1]
      vel[:, b] += term
      speed_bound[:, b] += np.sqrt(np.sum(np.asarray(term, np.float64)**2, axis=-1))

  # subtree sums, leaves first
  mass = np.array(body_mass, dt)
  mpos = xipos*body_mass[None, :, None]
  mvel = vel*body_mass[None, :, None]
  for b in range(nb - 1, 0, -1):
    par = int(m.body_parentid[b])
    mass[par] += mass[b]
    mpos[:, par] += mpos[:, b]
    mvel[:, par] += mvel[:, b]
  light = mass < dt(1e-15)
  safe = np.where(light, dt(1), mass)
  com = np.where(light[None, :, None], xipos, mpos/safe[None, :, None])
  linvel = np.where(light[None, :, None], dt(0), mvel/safe[None, :, None])
  f = Frames()
  f.xpos, f.xmat, f.xipos = xpos, xmat.reshape(bsz, nb, 9), xipos
  f.subtree_com, f.subtree_linvel = com, linvel
  f.body_speed_bound = speed_bound.max(axis=1)
  return f


# ---------------------------------------------------------------------------
# sensors, observation, reward
# ---------------------------------------------------------------------------
def sensors(m, frames, qpos, qvel):
  """-> sensordata [B, nsensordata], kinds [nsensordata] ('pos', 'vel', 'state'
  or 'touch': not modelled, NaN)."""
  n = int(m.nsensordata)
  out = np.full((len(qpos), max(n, 1)), np.nan, frames.xpos.dtype)
  kinds = ['touch']*max(n, 1)
  for s in range(int(m.nsensor)):
    kind, obj, adr = int(m.sensor_type[s]), int(m.sensor_objid[s]), int(m.sensor_adr[s])
    if kind == mdl.SENS_SUBTREELINVEL:
      out[:, adr:adr + 3], kinds[adr:adr + 3] = frames.subtree_linvel[:, obj], ['vel']*3
    elif kind == mdl.SENS_SUBTREECOM:
      out[:, adr:adr + 3], kinds[adr:adr + 3] = frames.subtree_com[:, obj], ['pos']*3
    elif kind == mdl.SENS_JOINTPOS:
      out[:, adr], kinds[adr] = qpos[:, int(m.jnt_qposadr[obj])], 'state'
    elif kind == mdl.SENS_JOINTVEL:
      out[:, adr], kinds[adr] = qvel[:, int(m.jnt_dofadr[obj])], 'state'
  return out, kinds


def _site(m, frames, spec):
  """World position of a `codegen.task_sites` entry."""
  body, local, _ = spec
  dt = frames.xpos.dtype.type
  local = np.asarray(local, np.float64).astype(dt)
  return frames.xpos[:, body] + _rot(frames.xmat[:, body].reshape(-1, 3, 3), local)


class Outputs:
  """What `evaluate` returns; see there."""


# One `tolerance()` term of a reward: its input x [B]; branch [B] (0 in bounds, 1
# on the slope, 2 on the floor: past the cut-off, or outside with margin 0);
# bounds (lower, upper) of a margin-0 term, else None; the tolerance class of x
# for such a term; the branches the term has at all.
Term = collections.namedtuple('Term', 'name x branch bounds kind reach')


def evaluate(model, task_id, task_param_i, task_param_r, qpos, qvel, ctrl, taskdata,
             dtype=np.float64):
  """The output stage for states qpos [B, nq], qvel [B, nv], controls ctrl
  [B, nu] and task data [B, ntaskdata] (or None).  -> Outputs with
    xpos, xipos, subtree_com, subtree_linvel [B, nbody, 3], xmat [B, nbody, 9]
    sensordata [B, nsensordata] (touch: NaN), sensor_kinds
    obs [B, nobs] in the kernel's order (touch: NaN), obs_kinds [nobs]
    reward [B]
    terms: [Term] per `tolerance()` term of the reward
  all in `dtype`."""
  m, dt = model, np.dtype(dtype).type
  c = lambda a: np.asarray(a, np.float64).astype(dt)
  qpos, qvel, ctrl = c(qpos), c(qvel), c(ctrl)
  f = kinematics(m, qpos, qvel, dtype)
  o = Outputs()
  o.xpos, o.xmat, o.xipos = f.xpos, f.xmat, f.xipos
  o.subtree_com, o.subtree_linvel = f.subtree_com, f.subtree_linvel
  o.body_speed_bound = f.body_speed_bound
  o.sensordata, o.sensor_kinds = sensors(m, f, qpos, qvel)
  bodies = codegen.task_bodies(m, task_id)
  sites = codegen.task_sites(m, task_id)
  nq, nv = int(m.nq), int(m.nv)
  state = lambda a: (a, ['state']*a.shape[1])
  zz = lambda b: f.xmat[:, b, 8]
  xz = lambda b: f.xmat[:, b, 2]
  parts, x_kinds = [], {}
  with task_formulas.recording() as rec:
    if task_id == codegen.TASK_CARTPOLE:
      poles = list(range(2, int(m.nbody)))
      trig = np.stack([g(p) for p in poles for g in (zz, xz)], axis=1)
      parts = [state(qpos[:, :1]), (trig, ['rot']*trig.shape[1]), state(qvel)]
      reward = task_formulas.cartpole_reward(
          qpos[:, 0], np.stack([zz(p) for p in poles], axis=1), ctrl[:, :1], qvel[:, 1:],
          sparse=bool(task_param_i & 1))
      x_kinds = {'cart': 'state', 'pole_cos': 'rot'}
    elif task_id == codegen.TASK_CHEETAH:
      parts = [state(qpos[:, 1:]), state(qvel)]
      reward = task_formulas.cheetah_reward(f.subtree_linvel[:, bodies[0], 0])
    elif task_id == codegen.TASK_HUMANOID:
      torso, head = bodies[0], bodies[1]
      rot = f.xmat[:, torso].reshape(-1, 3, 3)
      ext = [np.sum((f.xpos[:, b] - f.xpos[:, torso])[:, :, None]*rot, axis=1)
             for b in bodies[2:6]]
      cv = f.subtree_linvel[:, torso]
      parts = [state(qpos[:, 7:]), (f.xpos[:, head, 2:3], ['pos']),
               (np.concatenate(ext, axis=1), ['pos']*12), (rot[:, 2], ['rot']*3),
               (cv, ['vel']*3), state(qvel)]
      reward = task_formulas.humanoid_reward(
          f.xpos[:, head, 2], zz(torso), ctrl, cv, float(task_param_r[0]))
    elif task_id == codegen.TASK_WALKER:
      torso = bodies[0]
      orient = np.stack([f.xmat[:, b, k] for b in range(1, int(m.nbody)) for k in (0, 2)],
                        axis=1)
      parts = [(orient, ['rot']*orient.shape[1]), (f.xpos[:, torso, 2:3], ['pos']),
               state(qvel)]
      reward = task_formulas.walker_reward(
          f.xpos[:, torso, 2], zz(torso), f.subtree_linvel[:, torso, 0],
          float(task_param_r[0]))
    elif task_id == codegen.TASK_PENDULUM:
      pole = bodies[0]
      parts = [(np.stack([zz(pole), xz(pole)], axis=1), ['rot']*2), state(qvel[:, :1])]
      reward = task_formulas.pendulum_reward(zz(pole))
      x_kinds = {'pole_vertical': 'rot'}
    elif task_id == codegen.TASK_HOPPER:
      torso, foot = bodies
      ntouch = codegen.observation_size(m, task_id) - (nq - 1) - nv
      parts = [state(qpos[:, 1:]), state(qvel),
               (np.full((len(qpos), ntouch), np.nan, dt), ['touch']*ntouch)]
      reward = task_formulas.hopper_reward(
          f.xipos[:, torso, 2] - f.xipos[:, foot, 2], f.subtree_linvel[:, torso, 0], ctrl,
          bool(task_param_i & 1))
      x_kinds = {'height': 'pos'}
    elif task_id == codegen.TASK_POINTMASS:
      parts = [state(qpos), state(qvel)]
      d = _site(m, f, sites[1]) - _site(m, f, sites[0])
      reward = task_formulas.point_mass_reward(
          np.sqrt(np.sum(d*d, axis=1)), ctrl, target_size=dt(sites[1][2]))
    elif task_id == codegen.TASK_REACHER:
      to = c(taskdata)[:, :2] - _site(m, f, sites[0])[:, :2]
      parts = [state(qpos), (to, ['pos']*2), state(qvel)]
      reward = task_formulas.reacher_reward(
          np.sqrt(np.sum(to*to, axis=1)), dt(task_param_r[0]), finger_size=dt(0))
      x_kinds = {'finger_to_target': 'pos'}
    elif task_id == codegen.TASK_ACROBOT:
      upper, lower = bodies
      parts = [(np.stack([xz(upper), xz(lower), zz(upper), zz(lower)], axis=1), ['rot']*4),
               state(qvel)]
      d = _site(m, f, sites[1]) - _site(m, f, sites[0])
      reward = task_formulas.acrobot_reward(
          np.sqrt(np.sum(d*d, axis=1)), bool(task_param_i & 1),
          target_radius=dt(sites[1][2]))
      x_kinds = {'to_target': 'pos'}
    else:
      raise ValueError('no task layer for task %r' % (task_id,))
  o.obs = np.concatenate([p[0] for p in parts], axis=1)
  o.obs_kinds = [k for p in parts for k in p[1]]
  assert o.obs.shape[1] == codegen.observation_size(m, task_id) and o.obs.dtype == dt
  o.reward = np.asarray(reward, dt)
  assert np.asarray(reward).dtype == dt, np.asarray(reward).dtype
  o.terms = []
  for name, x, branch, bounds, margin, sigmoid in rec:
    x2 = np.asarray(x).reshape(len(qpos), -1)
    b2 = np.asarray(branch).reshape(len(qpos), -1)
    reach = (0, 2) if margin == 0 else (0, 1) if sigmoid == 'gaussian' else (0, 1, 2)
    for k in range(x2.shape[1]):
      label = name if x2.shape[1] == 1 else '%s[%d]' % (name, k)
      o.terms.append(Term(label, x2[:, k], b2[:, k], bounds if margin == 0 else None,
                          x_kinds.get(name), reach))
  return o


# the reference's observation keys in `get_observation` order with the width of
# each (suite/*.py of the reference, read by hand; cartpole and acrobot are also
# held by tasks.json) and the host task's own get_observation order
OBS_LAYOUT = {
    'cartpole': (('position', 3), ('velocity', 2)),
    'cheetah': (('position', 8), ('velocity', 9)),
    'humanoid': (('joint_angles', 21), ('head_height', 1), ('extremities', 12),
                 ('torso_vertical', 3), ('com_velocity', 3), ('velocity', 27)),
    'walker': (('orientations', 14), ('height', 1), ('velocity', 9)),
    'pendulum': (('orientation', 2), ('velocity', 1)),
    'acrobot': (('orientations', 4), ('velocity', 2)),
    'hopper': (('position', 6), ('velocity', 7), ('touch', 2)),
    'reacher': (('position', 2), ('to_target', 2), ('velocity', 2)),
    'point_mass': (('position', 2), ('velocity', 2)),
}


def obs_slices(domain):
  out, at = {}, 0
  for key, width in OBS_LAYOUT[domain]:
    out[key] = slice(at, at + width)
    at += width
  return out


def scales(out64):
  """{class: [B]} of the tolerance rule above, from a float64 `evaluate`."""
  n = len(out64.reward)
  return {'pos': np.maximum(1.0, np.abs(out64.xpos).reshape(n, -1).max(axis=1)),
          'rot': np.ones(n), 'reward': np.ones(n), 'state': np.zeros(n),
          'vel': np.maximum(1.0, out64.body_speed_bound)}


def classes(out):
  """{class: [(name, values [B, k])]}: every modelled output by tolerance
  class (touch entries left out)."""
  n = len(out.reward)
  by = {k: [] for k in CLASSES + ('state',)}
  by['pos'] += [('xpos', out.xpos.reshape(n, -1)), ('xipos', out.xipos.reshape(n, -1)),
                ('subtree_com', out.subtree_com.reshape(n, -1))]
  by['rot'].append(('xmat', out.xmat.reshape(n, -1)))
  by['vel'].append(('subtree_linvel', out.subtree_linvel.reshape(n, -1)))
  by['reward'].append(('reward', out.reward.reshape(n, 1)))
  for name, values, kinds in (('obs', out.obs, out.obs_kinds),
                              ('sensordata', out.sensordata, out.sensor_kinds)):
    kinds = np.array(kinds)
    for kind in by:
      if (kinds == kind).any():
        by[kind].append(('%s.%s' % (name, kind), values[:, kinds == kind]))
  return by


def excluded(out64, tol_of_kind):
  """[B] bool: the reward samples that may be left out: a margin-0 term's input
  within that input's own tolerance of one of its bounds.  tol_of_kind:
  {class: [B]} absolute tolerances."""
  out = np.zeros(len(out64.reward), bool)
  for term in out64.terms:
    if term.bounds is None:
      continue
    for bound in term.bounds:
      if np.isfinite(bound):
        out |= np.abs(np.asarray(term.x, np.float64) - bound) <= tol_of_kind[term.kind]
  return out


def fp32_tolerances(out64):
  """{class: [B]} absolute device bounds for fp32 / mixed code objects."""
  s = scales(out64)
  tol = {k: bound_in_eps(k)*EPS32*s[k] for k in CLASSES}
  tol['state'] = np.zeros(len(out64.reward))
  return tol
