"""Shared by the per-env model parameter tests: the perturbation of the issue and
the expected trajectory (always the fp64 oracle on a perturbed copy of the model)."""

import copy

import numpy as np

from dm_control_amd import codegen
from dm_control_amd.mjcf import compiler

ALL_FIELDS = codegen.PER_ENV_FIELDS


def perturbed(model, rs, fields=ALL_FIELDS):
  """deepcopy(model) with the fields in `fields` scaled by factors from `rs`
  (drawn for every field either way, so a field's factors do not depend on
  which others vary), then mj_setConst."""
  m = copy.deepcopy(model)
  fm = rs.uniform(0.7, 1.3, m.nbody)
  fi = rs.uniform(0.7, 1.3, m.nbody)
  fd, fa = rs.uniform(0.5, 2, m.nv), rs.uniform(0.5, 2, m.nv)
  fs = rs.uniform(0.5, 2, m.njnt)
  ff = rs.uniform(0.4, 1.2, m.ngeom)
  fg = rs.uniform(0.8, 1.2, m.nu)
  gg = rs.uniform(0.8, 1.2)
  fp = rs.uniform(0.8, 1.2, (2, m.nu))     # gain and bias parameters (drawn last)
  if 'body_mass' in fields:
    m.body_mass = m.body_mass*fm
  if 'body_inertia' in fields:
    m.body_inertia = m.body_inertia*fi[:, None]
  if 'dof_damping' in fields:
    m.dof_damping = m.dof_damping*fd
  if 'dof_armature' in fields:
    m.dof_armature = m.dof_armature*fa
  if 'jnt_stiffness' in fields:
    m.jnt_stiffness = m.jnt_stiffness*fs
  if 'geom_friction' in fields:
    m.geom_friction = np.array(m.geom_friction, float)
    m.geom_friction[:, 0] *= ff
  if 'actuator_gear' in fields and m.nu:
    m.actuator_gear = (np.asarray(m.actuator_gear).T*fg).T
  if 'actuator_gainprm' in fields and m.nu:
    m.actuator_gainprm = np.asarray(m.actuator_gainprm)*fp[0][:, None]
  if 'actuator_biasprm' in fields and m.nu:
    m.actuator_biasprm = np.asarray(m.actuator_biasprm)*fp[1][:, None]
  if 'gravity' in fields:
    m.opt.gravity = np.asarray(m.opt.gravity, float)*gg
  compiler._set_const(m)
  m.opt.meaninertia = m.meaninertia
  return m


# Two hinges driven by actuators WITH a bias term (biastype affine): a position
# servo (gain kp, bias (0, -kp, 0)) and a general actuator with all three bias
# parameters and a second gain entry that must stay unread; gears != 1, and one
# limited joint so that a constraint row is in play.  The only models of the
# suite with such actuators are the soccer walkers (team mode).
SERVO_ARM = """
<mujoco model='servo_arm'>
  <option timestep='0.002'/>
  <worldbody>
    <body name='upper' pos='0 0 1'>
      <joint name='shoulder' type='hinge' axis='0 1 0' damping='0.05' limited='true' range='-0.4 0.4'/>
      <geom name='upper' type='capsule' fromto='0 0 0 0.3 0 0' size='0.03' contype='0' conaffinity='0'/>
      <body name='lower' pos='0.3 0 0'>
        <joint name='elbow' type='hinge' axis='0 1 0' damping='0.02'/>
        <geom name='lower' type='capsule' fromto='0 0 0 0.25 0 0' size='0.02' contype='0' conaffinity='0'/>
      </body>
    </body>
  </worldbody>
  <actuator>
    <position name='shoulder' joint='shoulder' kp='12' gear='1.5'/>
    <general name='elbow' joint='elbow' gear='0.7' gainprm='3 0 0' biastype='affine' biasprm='0.4 -2.5 -0.3'/>
  </actuator>
</mujoco>
"""
ACTUATOR_FIELDS = ('actuator_gear', 'actuator_gainprm', 'actuator_biasprm')


def alternating_ctrl(nu):
  """A constant control of +0.5 and -0.5 in turn."""
  return np.array([-0.5 if i % 2 else 0.5 for i in range(nu)])


def block_of(m, layout):
  return codegen.model_param_values(m, layout)


ONE_LANE_DOMAINS = ('cartpole', 'cheetah', 'hopper', 'walker', 'pendulum', 'acrobot')
COOP_DOMAINS = ('cheetah', 'walker', 'humanoid')


def gpu_shapes():
  """(domain, precision, mode, group, lds_budget) of the varied builds the GPU
  tests run, read off tests/selection_matrix.py: every fp32 / fp64
  one-env-per-lane line (all three LDS budgets) of the one-lane domains and
  every several-lanes line of the several-lanes domains."""
  import selection_matrix as sm
  one, coop = [], []
  for domain, precision, mode, group, lds, _, _ in sm.SHIPPED:
    if precision not in ('f32', 'f64'):
      continue
    if mode == 'auto' and domain in ONE_LANE_DOMAINS:
      one.append((domain, precision, 'auto', 64, lds))
    elif mode == 'coop' and domain in COOP_DOMAINS:
      coop.append((domain, precision, 'coop', group, None))
  return one + coop


def gpu_builds():
  """[(model, task, build_model kwargs)] of every varied code object the GPU tests load."""
  import helpers
  import kat_models
  out = [(helpers.load_model(d), helpers.TASKS[d],
          dict(precision=p, mode=mode, group=group, lds_budget=lds, per_env=ALL_FIELDS))
         for d, p, mode, group, lds in gpu_shapes()]
  ball = compiler.from_xml_string(kat_models.BALL_ON_FLOOR)
  out.append((ball, 0, dict(precision='f64', per_env=('gravity',))))
  servo = compiler.from_xml_string(SERVO_ARM)
  for mode, group in (('auto', 64), ('coop', 64)):
    out.append((servo, 0, dict(precision='f64', mode=mode, group=group, per_env=ACTUATOR_FIELDS)))
  return out
