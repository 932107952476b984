"""Host side of the per-env model parameters (DMC_FIELD_MODELPARAM).

A build with `per_env` fields reads those fields, and the constants that follow
from them, from a block of `[row][nenv]` values (codegen.model_param_layout).
`ModelParams` keeps the fp64 values of every env on the host, takes the user's
writes (broadcast, `envs=` selection), recomputes what `mj_setConst` would --
for all envs at once -- and packs the block that goes to the device.  Pure
numpy: no device, no library.
"""

import numpy as np

from dm_control_amd import codegen
from dm_control_amd.mjcf import compiler
from dm_control_amd.mjcf import model as mdl

# user-facing field -> trailing shape as a function of the model
_SHAPES = {
    'body_mass': lambda m: (m.nbody,), 'body_inertia': lambda m: (m.nbody, 3),
    'dof_damping': lambda m: (m.nv,), 'dof_armature': lambda m: (m.nv,),
    'jnt_stiffness': lambda m: (m.njnt,), 'actuator_gear': lambda m: (m.nu,),
    'actuator_gainprm': lambda m: (m.nu, 3), 'actuator_biasprm': lambda m: (m.nu, 3),
    'geom_friction': lambda m: (m.ngeom, 3), 'gravity': lambda m: (3,),
}


def _model_value(m, name):
  v = m.opt.gravity if name == 'gravity' else getattr(m, name)
  return np.asarray(v, np.float64).reshape(_SHAPES[name](m))


class NotPositiveDefinite(ValueError):
  """`envs`: the envs whose mass matrix at qpos0 is not positive definite."""

  def __init__(self, envs, note=''):
    self.envs = [int(e) for e in envs]
    ValueError.__init__(self, 'mass matrix at qpos0 is not positive definite for env(s) %s%s'
                        % (', '.join(map(str, self.envs)), note))


class SetConst:
  """`compiler._set_const` for many parameter sets of one model at once.

  The Jacobians at `qpos0` do not depend on masses, inertias or armatures, and
  the mass matrix is linear in them: M_e = diag(armature_e) + sum_b mass_eb A_b
  + sum_bk inertia_ebk c_bk c_bk^T.  One einsum and one batched inverse replace
  a Python pass per env (1.4 ms per cheetah, 7 ms per humanoid)."""

  def __init__(self, m):
    self.m = m
    self.pairs = codegen.collision_pairs(m)
    if m.nv == 0:
      return
    xpos, _, xmat, xipos, ximat, xanchor, xaxis = compiler.kinematics_qpos0(m)
    jacs = np.array([compiler._body_jacobian(m, b, xipos[b], xmat, xanchor, xaxis, xpos)
                     for b in range(m.nbody)])              # [nbody, 6, nv]
    self.jacs = jacs
    self.A = np.einsum('bki,bkj->bij', jacs[:, :3], jacs[:, :3])
    # principal axes of the bodies' inertias in the world, through the Jacobian
    self.C = np.einsum('bri,brk->bki', jacs[:, 3:], ximat)  # [nbody, 3, nv]
    self.welded = np.asarray(m.body_weldid) == 0

  def __call__(self, mass, inertia, armature, friction):
    """mass [E, nbody], inertia [E, nbody, 3], armature [E, nv], friction
    [E, ngeom, 3] -> dict of derived rows; raises ValueError naming the envs
    (positions in the arrays given) whose mass matrix is not positive definite."""
    m = self.m
    E = mass.shape[0]
    sub = mass.copy()
    for i in range(m.nbody - 1, 0, -1):
      sub[:, m.body_parentid[i]] += sub[:, i]
    out = {'body_subtreemass': sub}
    binv = np.zeros((E, m.nbody, 2))
    if m.nv == 0:
      out.update(dof_invweight0=np.zeros((E, 0)), meaninertia=np.ones(E))
    else:
      live = (mass != 0)
      live[:, 0] = False                    # (the world; massless bodies add nothing)
      mm = np.einsum('eb,bij->eij', mass*live, self.A)
      mm += np.einsum('ebk,bki,bkj->eij', inertia*live[:, :, None], self.C, self.C)
      idx = np.arange(m.nv)
      mm[:, idx, idx] += armature
      with np.errstate(all='ignore'):
        eig = np.linalg.eigvalsh(mm)
      bad = np.nonzero(~(np.all(np.isfinite(eig), axis=1) & np.all(eig > 0, axis=1)))[0]
      if len(bad):
        raise NotPositiveDefinite(bad)
      minv = np.linalg.inv(mm)
      diag = minv[:, idx, idx].copy()
      for j in range(m.njnt):
        a, t = int(m.jnt_dofadr[j]), int(m.jnt_type[j])
        if t == mdl.JNT_FREE:
          diag[:, a:a + 3] = diag[:, a:a + 3].mean(axis=1, keepdims=True)
          diag[:, a + 3:a + 6] = diag[:, a + 3:a + 6].mean(axis=1, keepdims=True)
        elif t == mdl.JNT_BALL:
          diag[:, a:a + 3] = diag[:, a:a + 3].mean(axis=1, keepdims=True)
      out['dof_invweight0'] = np.maximum(diag, mdl.MJ_MINVAL)
      out['meaninertia'] = mm[:, idx, idx].mean(axis=1)
      for half in (0, 1):
        J = self.jacs[:, 3*half:3*half + 3]
        tr = np.einsum('bki,eij,bkj->eb', J, minv, J)/3
        binv[:, :, half] = np.maximum(mdl.MJ_MINVAL, tr)
      binv[:, self.welded] = 0
      binv[:, 0] = 0
    out['body_invweight0'] = binv
    out['pair_diag'] = self.pair_diag(binv, friction)
    return out

  def pair_friction(self, friction):
    """[E, ngeom, 3] -> [E, npair, 5], mixed as codegen.mix_pair does."""
    m = self.m
    out = np.zeros((friction.shape[0], len(self.pairs), 5))
    for p, (g1, g2) in enumerate(self.pairs):
      if m.geom_priority[g1] != m.geom_priority[g2]:
        f = friction[:, g1 if m.geom_priority[g1] > m.geom_priority[g2] else g2]
      else:
        f = np.maximum(friction[:, g1], friction[:, g2])
      out[:, p] = f[:, [0, 0, 1, 2, 2]]
    return out

  def pair_diag(self, binv, friction):
    m = self.m
    fr = self.pair_friction(friction)
    out = np.zeros((binv.shape[0], len(self.pairs), 6))
    for p, (g1, g2) in enumerate(self.pairs):
      b1, b2 = int(m.geom_bodyid[g1]), int(m.geom_bodyid[g2])
      tran = binv[:, b1, 0] + binv[:, b2, 0]
      rot = binv[:, b1, 1] + binv[:, b2, 1]
      out[:, p, 0] = tran
      for k in range(5):
        out[:, p, 1 + k] = tran + fr[:, p, k]*fr[:, p, k]*(tran if k < 2 else rot)
    return out


class ModelParams:
  """fp64 values of the per-env fields of a batch and their packing."""

  def __init__(self, model, per_env, nenv):
    self.model = model
    self.per_env = codegen.normalise_per_env(per_env)
    self.nenv = int(nenv)
    self.layout = codegen.model_param_layout(model, self.per_env)
    self.nrows = sum(n for _, n in self.layout.values())
    self._const = SetConst(model) if self.per_env else None
    # every field, varied or not (the derived rows need them all) -- of a batch
    # that varies something: a default batch keeps no copies
    self.values = {}
    if self.per_env:
      self.values = {name: np.tile(_model_value(model, name), (self.nenv,) + (1,)*len(_SHAPES[name](model)))
                     for name in _SHAPES}
    self.derived = {}
    if self.per_env:
      npair = len(self._const.pairs)
      one = lambda v, shape: np.tile(np.asarray(v, np.float64).reshape(shape), (self.nenv,) + (1,)*len(shape))
      fric, diag = codegen.pair_rows(model, self._const.pairs)
      self.derived = {
          'body_subtreemass': one(model.body_subtreemass, (model.nbody,)),
          'dof_invweight0': one(model.dof_invweight0, (model.nv,)),
          'meaninertia': np.full(self.nenv, float(model.meaninertia)),
          'pair_diag': one(diag, (npair, 6))}

  def _envs(self, envs):
    if envs is None:
      return np.arange(self.nenv)
    envs = np.asarray(envs)
    if envs.dtype == bool:
      if envs.shape != (self.nenv,):
        raise ValueError('envs: a mask must have shape (%d,), got %r' % (self.nenv, envs.shape))
      return np.nonzero(envs)[0]
    envs = np.atleast_1d(envs).astype(np.int64)
    if envs.ndim != 1 or np.any(envs < -self.nenv) or np.any(envs >= self.nenv):
      raise ValueError('envs: indices must lie in [0, %d)' % self.nenv)
    return envs % self.nenv

  def check_field(self, name):
    name = 'gravity' if name == 'opt.gravity' else name
    if name not in self.per_env:
      raise ValueError(
          'the compiled model is immutable: what a task varies per episode is '
          'per-instance task data (DMC_FIELD_TASKDATA), see suite/reacher.py.  '
          'Fields named in the `per_env` argument of Physics (%s) can be written '
          'per env; %r is not among this batch\'s (%s).'
          % (', '.join(codegen.PER_ENV_FIELDS), name, ', '.join(self.per_env) or 'none'))
    return name

  def set(self, fields, envs=None, set_const=True):
    """Takes {field: array [B', ...] or [...] (broadcast over the selected envs)};
    returns the whole block [nrows, nenv] (fp64) to be written to the device."""
    for name in fields:
      self.check_field(name)
    sel = self._envs(envs)
    new = {}
    for name, value in fields.items():
      name = self.check_field(name)
      shape = _SHAPES[name](self.model)
      value = np.asarray(value, np.float64)
      if value.shape not in (shape, (len(sel),) + shape):
        raise ValueError('%s: expected shape %r or %r, got %r'
                         % (name, shape, (len(sel),) + shape, value.shape))
      if not np.all(np.isfinite(value)):
        raise ValueError('%s: values must be finite' % name)
      new[name] = np.broadcast_to(value, (len(sel),) + shape)
    trial = {name: (new[name] if name in new else self.values[name][sel]) for name in _SHAPES}
    derived = None
    if set_const and self.per_env and len(sel):
      try:
        derived = self._const(trial['body_mass'], trial['body_inertia'],
                              trial['dof_armature'], trial['geom_friction'])
      except NotPositiveDefinite as e:      # positions in the selection -> env ids
        raise NotPositiveDefinite([sel[t] for t in e.envs], '; nothing was written')
    for name in new:
      self.values[name][sel] = new[name]
    if derived is not None:
      for name in self.derived:
        self.derived[name][sel] = derived[name]
    return self.block()

  def get(self, name):
    name = 'gravity' if name == 'opt.gravity' else name
    if name in self.derived:
      return self.derived[name].copy()
    if name not in _SHAPES:
      raise ValueError('unknown model parameter %r' % name)
    if not self.per_env:      # nothing varies: the compiled model's value in every env
      v = _model_value(self.model, name)
      return np.tile(v, (self.nenv,) + (1,)*v.ndim)
    return self.values[name].copy()

  def block(self):
    out = np.zeros((max(self.nrows, 1), self.nenv))
    for name, (o, n) in self.layout.items():
      if name == 'pair_friction':
        v = self._const.pair_friction(self.values['geom_friction'])
      elif name in self.derived:
        v = self.derived[name]
      else:
        v = self.values[name]
      out[o:o + n] = v.reshape(self.nenv, n).T
    return out

  def load_block(self, block, values):
    """Checkpoint restore: `values` {field: [B, ...]}, derived rows from `block`."""
    for name in _SHAPES:
      if name in values:
        self.values[name][...] = values[name]
    for name in self.derived:
      o, n = self.layout[name]
      self.derived[name][...] = np.asarray(block[o:o + n], np.float64).T.reshape(self.derived[name].shape)
