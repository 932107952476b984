"""States at and around the contact capacity ("at capacity").

Every other test stays below `ncon_max`; the ones that import this module build
with a small cap K and step envs whose TRUE contact count (the oracle's with
room for all of them) is K-1, K, K+1 and >= K+4.  The states are those of
`helpers.initial_states` (shallow penetration), three out of four pressed
further into the floor and rolled so that the count is spread out, one of
eight raised again until its count is next to a cap.
tests/test_capacity_cases.py checks, with the oracle alone, that the cases are
what the device tests need: the spread, that a wrong kept set is visible in the
velocities, and that no state sits where an fp32 build may legitimately count
differently."""

import copy
import functools

import numpy as np

import helpers
from oracle import oracle

NENV = 129
SEED = 7
# (model, cap K): 2 and 4 for the planar models, 8 for the humanoid
CASES = [('cheetah', 2), ('cheetah', 4), ('walker', 2), ('walker', 4),
         ('hopper', 2), ('hopper', 4), ('humanoid', 8)]
# the humanoid at the cap its default build gets (codegen.capacities: min(worst, 32))
DEFAULT_CAP = 32
DEFAULT_CAP_DRAWS = 10000
DEFAULT_CAP_SEED = 2026
NEAR_MARGIN = 1e-4
# The code objects of tests/test_gpu_capacity.py: (model, cap or None for the
# default build, build_model keywords).  Mode "auto" is the unrolled one-lane
# kernel in fp32 and "mixed"; in fp64 the unrolled cheetah exceeds the spill
# budget (as its default build does), so "auto" and "rolled" both resolve to
# the generic source and there is one fp64 line.  Not here, because
# `build_model` refuses them and no over-budget build runs at capacity: the
# humanoid with 128 lanes at K = 8 in fp64 (877 spilled VGPRs; its build at the
# default cap is within budget and is below).
GPU_BUILDS = [
    ('cheetah', 4, dict(precision='f32', mode='auto')),
    ('cheetah', 4, dict(precision='mixed', mode='auto')),
    ('cheetah', 4, dict(precision='f64', mode='rolled')),
    ('cheetah', 2, dict(precision='f32', mode='auto')),
    ('cheetah', 2, dict(precision='f64', mode='rolled')),
    ('hopper', 4, dict(precision='f64', mode='coop', group=16)),
    ('hopper', 2, dict(precision='f64', mode='coop', group=16)),
    ('walker', 4, dict(precision='f32', mode='coop', group=8)),
    ('walker', 2, dict(precision='f32', mode='coop', group=8)),
    ('humanoid', 8, dict(precision='f64', mode='coop', group=32)),
    ('humanoid', 8, dict(precision='f32', mode='coop', group=64)),
    # what `Physics` selects for the humanoid, at the cap codegen gives it
    ('humanoid', None, dict(precision='f32', mode='coop', group=128)),
    ('humanoid', None, dict(precision='f64', mode='coop', group=128))]
# Team mode (one wavefront per env, what `locomotion.soccer` runs): two walkers
# pushed into each other with the ball between their feet, TEAM_NCON contacts
# (tests/test_capacity_cases.py holds the oracle to the number); caps far
# below, one below, at and one above.  The strictly rolled tier: verdict "ok".
TEAM_NCON = 28
TEAM_CAPS = (5, TEAM_NCON - 1, TEAM_NCON, TEAM_NCON + 1)
TEAM_BUILD = dict(precision='f64', mode='team')
# WARN bits of the kernels (csrc/dmc_args.h) from the oracle's warning counters
WARN_CONTACTFULL, WARN_CNSTRFULL = 2, 4

# per model: index of the root height and of the root pitch in qpos, and per
# variant (env % 4) how far the root is pressed down and how far it is rolled
_ROOT = {'cheetah': (1, 2), 'walker': (0, 2), 'hopper': (1, 2)}
_PRESS = {'cheetah': (0.0, 0.25, 0.45, 0.6), 'walker': (0.0, 0.15, 0.5, 0.9),
          'hopper': (0.0, 0.1, 0.6, 1.05), 'humanoid': (0.0, 0.45, 0.7, 0.95)}
_ROLL = {'cheetah': (0.0, 0.0, 0.9, 1.5), 'walker': (0.0, 0.0, 0.9, 1.5),
         'hopper': (0.0, 0.0, 1.0, 1.55), 'humanoid': (0.0, 0.0, 0.7, 1.4)}
# a state that fails condition b) or c) is moved down or up by these steps until both hold
_NUDGE = tuple(s*0.003*k for k in range(12) for s in ((1, -1) if k else (1,)))
# ... and, if none of them does, rolled further by these angles
_TILT = (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0)
# envs e % 8 == 7 are raised from their variant in steps of _RISE until the true
# count is the next of the model's K-1, K, K+1: the buckets next to a cap hold
# enough envs whatever the spread of the others
_RISE = 0.004
_RISE_MAX = 1.3


def _quat_mul(a, b):
  w1, x1, y1, z1 = a
  w2, x2, y2, z2 = b
  return np.array([w1*w2 - x1*x2 - y1*y2 - z1*z2, w1*x2 + x1*w2 + y1*z2 - z1*y2,
                   w1*y2 - x1*z2 + y1*w2 + z1*x2, w1*z2 + x1*y2 - y1*x2 + z1*w2])


def _variant(name, q, e, nudge, tilt=0.0):
  """State e of `helpers.initial_states` as variant e % 4: pressed and rolled."""
  q = q.copy()
  v = e % 4
  sign = 1.0 if (e//4) % 2 else -1.0
  if name == 'humanoid':
    q[2] -= _PRESS[name][v] + nudge
    half = 0.5*sign*(_ROLL[name][v] + tilt)
    axis = (1.0, 0.0, 0.0) if (e//8) % 2 else (0.0, 1.0, 0.0)
    q[3:7] = _quat_mul(np.r_[np.cos(half), np.sin(half)*np.array(axis)], q[3:7])
  else:
    z, pitch = _ROOT[name]
    q[z] -= _PRESS[name][v] + nudge
    q[pitch] += sign*(_ROLL[name][v] + tilt)
  return q


def oracle_model(model, ncon_max=None, nefc_max=None):
  """The oracle of `model`, with `nconmax` / `nefcmax` set where given."""
  om = oracle.OracleModel(model)
  if ncon_max is not None:
    om.set_int('nconmax', ncon_max)
  if nefc_max is not None:
    om.set_int('nefcmax', nefc_max)
  return om


def at(om, qpos, qvel, ctrl=None):
  """OracleData of `om` at the state, after step1 (contacts and rows made)."""
  d = oracle.OracleData(om)
  d.qpos[:] = qpos
  d.qvel[:] = qvel
  if ctrl is not None:
    d.ctrl[:] = ctrl
  d.step1()
  return d


def _widened(model):
  """`model` with every geom margin at 2*NEAR_MARGIN: its contact list holds
  every candidate whose distance is below the true margin (0) + NEAR_MARGIN."""
  wide = copy.copy(model)
  wide.geom_margin = np.full_like(np.asarray(model.geom_margin, float), 2*NEAR_MARGIN)
  return wide


def near_margin(d_wide):
  """A candidate contact within NEAR_MARGIN of the pair's margin (0 in these
  models), in the oracle of the widened model."""
  return any(abs(d_wide.contact(c)['dist']) < NEAR_MARGIN for c in range(d_wide.ncon))


def admissible(model, om, om_wide, capped, qpos, qvel):
  """Conditions b) and c) on one state, against every cap of `capped`
  ({K: oracle model}): no candidate within NEAR_MARGIN of the margin, no
  capsule pair with crossing axes among the contacts (kept at any cap: among
  all), and where the state saturates a cap, the capped step differs from the
  uncapped one by more than 1e-3 in qvel."""
  if near_margin(at(om_wide, qpos, qvel)):
    return False
  d = at(om, qpos, qvel)
  if helpers._degenerate(d, model):
    return False
  full = expected(om, qpos, qvel, None)[4]
  return all(np.abs(expected(omk, qpos, qvel, None)[4] - full).max() > 1e-3
             for K, omk in capped.items() if d.ncon > K)


@functools.lru_cache(maxsize=None)
def states(name):
  """(model, qpos [NENV, nq], qvel [NENV, nv], true contact count [NENV])."""
  model = helpers.load_model(name)
  base_q, qvel = helpers.initial_states(model, name, NENV, seed=SEED)
  om, om_wide = oracle_model(model), oracle_model(_widened(model))
  caps = [K for n, K in CASES if n == name]
  capped = {K: oracle_model(model, K) for K in caps}
  targets = sorted(set(K + i for K in caps for i in (-1, 0, 1)))
  qpos = np.empty_like(base_q)
  count = np.zeros(NENV, int)
  rise = -np.arange(0.0, _RISE_MAX, _RISE)

  def counts(want):
    """The candidate has exactly `want` contacts (a tuned env)."""
    return lambda n: n == want

  def stays_far_above(n0):
    """The candidate is >= K+4 for every cap K for which the unmoved state
    (n0 contacts) is: an env far above a cap stays far above it."""
    return lambda n: all(n >= K + 4 for K in caps if n0 >= K + 4)

  for e in range(NENV):
    # (what the count must satisfy, offsets to try, extra roll): a tuned env goes
    # through the targets from its own on, and ends like any other env
    n0 = at(om, _variant(name, base_q[e], e, 0.0), qvel[e]).ncon
    tries = [(stays_far_above(n0), _NUDGE, tilt) for tilt in _TILT]
    if e % 8 == 7:
      tries = [(counts(targets[(e//8 + i) % len(targets)]), rise, 0.0)
               for i in range(len(targets))] + tries
    q = None
    for accepts, nudges, tilt in tries:
      for nudge in nudges:
        cand = _variant(name, base_q[e], e, nudge, tilt)
        if accepts(at(om, cand, qvel[e]).ncon) and admissible(
            model, om, om_wide, capped, cand, qvel[e]):
          q = cand
          break
      if q is not None:
        break
    assert q is not None, '%s env %d: no admissible state' % (name, e)
    qpos[e] = q
    count[e] = at(om, q, qvel[e]).ncon
  for a in (qpos, qvel, count):
    a.setflags(write=False)
  return model, qpos, qvel, count


def _lying(model, rs):
  """One draw of the default-cap search: full joint ranges, any orientation,
  root height near the floor."""
  q = np.array(model.qpos0, float)
  for j in range(model.njnt):
    if model.jnt_limited[j]:
      lo, hi = model.jnt_range[j]
      q[model.jnt_qposadr[j]] = rs.uniform(lo, hi)
  quat = rs.randn(4)
  q[3:7] = quat/np.linalg.norm(quat)
  q[2] = rs.uniform(0.02, 0.25)
  return q, 0.3*rs.randn(model.nv)


@functools.lru_cache(maxsize=None)
def default_cap_states():
  """The humanoid at DEFAULT_CAP: (model, qpos, qvel, true count) of NENV
  admissible draws of `_lying`, the ones with the most contacts in the middle
  of the batch; the search is DEFAULT_CAP_DRAWS draws of a fixed seed."""
  model = helpers.load_model('humanoid')
  om, om_wide = oracle_model(model), oracle_model(_widened(model))
  rs = np.random.RandomState(DEFAULT_CAP_SEED)
  found = []
  for _ in range(DEFAULT_CAP_DRAWS):
    q, v = _lying(model, rs)
    n = at(om, q, v).ncon
    if n >= DEFAULT_CAP - 4:
      found.append((n, q, v))
  capped = {DEFAULT_CAP: oracle_model(model, DEFAULT_CAP)}
  found = [f for f in found if admissible(model, om, om_wide, capped, f[1], f[2])]
  # up to four draws per count, from the fullest down
  found.sort(key=lambda f: -f[0])
  found = [f for i, f in enumerate(found) if sum(g[0] == f[0] for g in found[:i]) < 4]
  _, base_q, base_v, _ = states('humanoid')
  qpos, qvel = base_q.copy(), base_v.copy()
  count = np.array([at(om, q, v).ncon for q, v in zip(qpos, qvel)])
  slots = [e for e in range(NENV) if e % 4 == 1][:len(found)]
  for e, (n, q, v) in zip(slots, found):
    qpos[e], qvel[e], count[e] = q, v, n
  for a in (qpos, qvel, count):
    a.setflags(write=False)
  return model, qpos, qvel, count


def team_scene():
  """(model, qpos, qvel) of the team-mode case: the scene of
  tests/test_kernel_sanitizers.py with contacts between the two trees."""
  import test_kernel_sanitizers
  return test_kernel_sanitizers._team_scene('two_walkers_touching')   # pylint: disable=protected-access


def expected(om, qpos, qvel, ctrl):
  """One step of the oracle `om` (capped or not) from the state: (ncon, nefc,
  warn bits, qpos, qvel after the step, the oracle's warning counters)."""
  d = at(om, qpos, qvel, ctrl)
  ncon, nefc = d.ncon, d.nefc
  warn = (WARN_CONTACTFULL if d.warning[1] else 0) | (WARN_CNSTRFULL if d.warning[2] else 0)
  d.step2()
  return ncon, nefc, warn, d.qpos.copy(), d.qvel.copy(), d.warning.copy()


def envs_at(count, K):
  """Env indices by true count: {'K-1', 'K', 'K+1', '>=K+4'}."""
  return {'K-1': np.flatnonzero(count == K - 1), 'K': np.flatnonzero(count == K),
          'K+1': np.flatnonzero(count == K + 1), '>=K+4': np.flatnonzero(count >= K + 4)}
