"""The kernel SOURCES at contact and row capacity, on the host under sanitizers.

Every other test stays below `ncon_max` / `nefc_max`.  Here each kernel shape is
built through tests/shim_runner.py with a small cap K and stepped from the
states of tests/capacity_cases.py, whose true contact count is K-1, K, K+1 and
>= K+4, next to the oracle with `nconmax = K` ("at capacity"):
the kept set is the first K contacts in pair order, stats[0] and the CONTACTFULL
bit are the oracle's, the step is the capped oracle's step, an env next to a
saturated one computes what it computes next to an airborne one, and every
index stays inside buffers that hold exactly the envs of the program
(AddressSanitizer; ThreadSanitizer on shapes of several lanes).  The row
capacity is cut by `nefc_max`, which no product build sets.
"""

import numpy as np
import pytest

import capacity_cases as cc
import helpers
import shim_runner
from dm_control_amd import codegen

STEPS = 2
BUCKETS = ('K-1', '>=K+4', 'K', 'K+1')


def _ctrl(model):
  return 0.5*np.cos(np.arange(model.nu))


def _programs(count, K, nenv):
  """Env indices of each run of a program that holds `nenv` envs, so that the
  runs together step an env of every bucket; where a program holds several, a
  saturated env sits between unsaturated ones."""
  by = cc.envs_at(count, K)
  order = [by[BUCKETS[i % 4]][i//4] for i in range(max(4, nenv))]
  return [order[i:i + nenv] for i in range(0, len(order) - nenv + 1, nenv)]


def _step_and_compare(exe, model, qpos, qvel, envs, K, nefc_max=None, steps=STEPS, timeout=600):
  ctrl = _ctrl(model)
  rows = shim_runner.run(exe, steps, qpos[envs], qvel[envs], ctrl, timeout=timeout)
  shim_runner.compare(rows, [model]*len(envs), qpos[envs], qvel[envs], ctrl, steps,
                      expect=dict(ncon_max=K, nefc_max=nefc_max))
  return rows


def _check_case(exe, name, K, nenv, default_cap=False, timeout=600):
  """Every bucket of the case on the program, and the neighbours of the
  saturated envs against a run with airborne envs in their place."""
  model, qpos, qvel, count = cc.default_cap_states() if default_cap else cc.states(name)
  airborne = int(np.flatnonzero(count == 0)[0])
  seen = set()
  for envs in _programs(count, K, nenv):
    envs = np.array(envs)
    rows = _step_and_compare(exe, model, qpos, qvel, envs, K, timeout=timeout)
    for (e, _, (ncon, _, _, warn)) in rows[:len(envs)]:
      assert ncon == min(count[envs[e]], K)
      assert warn == (cc.WARN_CONTACTFULL if count[envs[e]] > K else 0)
      seen.add((min(count[envs[e]], K + 4) - K))
    if nenv > 1:
      full = count[envs] > K
      assert full.any() and not full.all()
      twin = np.where(full, airborne, envs)
      rows_twin = _step_and_compare(exe, model, qpos, qvel, twin, K, timeout=timeout)
      for a, b in zip(rows, rows_twin):
        if not full[a[0]]:
          assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], a[0]
  assert seen == {-1, 0, 1, 4}


# ---------------------------------------------------------------------------
# one env per lane (csrc/dmc_kernels.hip)
# ---------------------------------------------------------------------------
@pytest.mark.timeout(1200)
@pytest.mark.parametrize('name,K,unroll,extra', [
    ('cheetah', 2, True, ()), ('cheetah', 4, False, ()),
    ('hopper', 4, True, ()), ('hopper', 2, False, ()),
    # the contact list straddles the LDS and the HBM tier at saturation
    ('cheetah', 4, True, ('-DDMC_CON_LDS=2',)), ('hopper', 4, False, ('-DDMC_CON_LDS=3',)),
    ('hopper', 2, True, ('-DDMC_CON_LDS=1',)),
    # packed matrices in the HBM workspace
    ('cheetah', 4, False, ('-DDMC_MAT_PRIVATE_BYTES=64',)),
    ('hopper', 2, False, ('-DDMC_MAT_PRIVATE_BYTES=64', '-DDMC_CON_LDS=1'))])
def test_one_lane_source_at_contact_capacity(name, K, unroll, extra, tmp_path):
  model = cc.states(name)[0]
  exe = shim_runner.build(model, helpers.TASKS[name], tmp_path, unroll=unroll, ncon_max=K,
                          extra=extra)
  _check_case(exe, name, K, 1)


def _stacked_boxes():
  model, task, q, v, _ = shim_runner.case('stacked_boxes')
  return model, task, q, v, shim_runner.oracle_at(model, q[0], v[0], np.zeros(model.nu)).ncon


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('unroll', [True, False])
def test_one_lane_source_cuts_a_box_manifold_at_capacity(unroll, tmp_path):
  """`stacked_boxes` (4-point manifolds, 8 contacts at the start): a cap inside
  the second manifold, one below the count, the count itself (no warning) and
  one above."""
  model, task, q, v, ncon = _stacked_boxes()
  assert ncon == 8
  ctrl = np.zeros(model.nu)
  for K in (6, ncon - 1, ncon, ncon + 1):
    exe = shim_runner.build(model, task, tmp_path, unroll=unroll, ncon_max=K, name='k%d' % K)
    rows = shim_runner.run(exe, STEPS, q, v, ctrl)
    shim_runner.compare(rows, [model], q, v, ctrl, STEPS, expect=dict(ncon_max=K))
    assert rows[0][2][0] == min(K, ncon)
    assert rows[0][2][3] == (cc.WARN_CONTACTFULL if K < ncon else 0)


# ---------------------------------------------------------------------------
# several lanes per env (csrc/dmc_coop.hip): one OS thread per lane
# ---------------------------------------------------------------------------
@pytest.mark.timeout(2400)
@pytest.mark.parametrize('name,K,group,sanitizer,default_cap', [
    ('walker', 2, 8, 'address,undefined', False), ('walker', 4, 8, 'thread', False),
    ('hopper', 4, 16, 'address,undefined', False), ('hopper', 2, 16, 'thread', False),
    ('cheetah', 4, 32, 'address,undefined', False), ('cheetah', 2, 32, 'thread', False),
    ('humanoid', 8, 64, 'address,undefined', False),
    ('humanoid', 8, 128, 'thread', False), ('humanoid', 8, 128, 'address,undefined', False),
    ('humanoid', cc.DEFAULT_CAP, 64, 'address,undefined', True),
    ('humanoid', cc.DEFAULT_CAP, 128, 'thread', True)])
def test_several_lanes_source_at_contact_capacity(name, K, group, sanitizer, default_cap, tmp_path):
  model = cc.states(name)[0]
  exe = shim_runner.build(model, helpers.TASKS[name], tmp_path, group=group, sanitizer=sanitizer,
                          ncon_max=None if default_cap else K)
  _check_case(exe, name, K, max(1, 64//group), default_cap, timeout=2000)


# ---------------------------------------------------------------------------
# team mode (csrc/dmc_kernels.hip, -DDMC_TEAM)
# ---------------------------------------------------------------------------
@pytest.mark.timeout(2400)
@pytest.mark.parametrize('sanitizer', ['address,undefined', 'thread'])
def test_team_source_at_contact_capacity(sanitizer, tmp_path):
  """Two walkers and the ball, pushed into each other: caps far below, one
  below, at and one above the scene's contact count.  The dropped contacts
  include the ones between the trees (the last pairs of the list)."""
  m, qpos, qvel = cc.team_scene()
  ctrl = np.zeros(m.nu)
  ncon = shim_runner.oracle_at(m, qpos, qvel, ctrl).ncon
  assert ncon == cc.TEAM_NCON
  for K in cc.TEAM_CAPS:
    exe = shim_runner.build(m, 0, tmp_path, unroll=False, team=8, ncon_max=K, sanitizer=sanitizer,
                            name='k%d' % K)
    rows = shim_runner.run(exe, 1, qpos[None], qvel[None], ctrl, timeout=2000)
    shim_runner.compare(rows, [m], qpos[None], qvel[None], ctrl, 1, expect=dict(ncon_max=K))
    assert rows[0][2][0] == min(K, ncon)
    assert rows[0][2][3] == (cc.WARN_CONTACTFULL if K < ncon else 0)


# ---------------------------------------------------------------------------
# the optional row capacity of codegen
# ---------------------------------------------------------------------------
def test_headers_are_unchanged_without_a_row_capacity():
  """`nefc_max=None` is the header without the argument: every suite model and
  task, rolled and unrolled (one code path today: this pins the default against
  a later edit that gives None a meaning of its own); a given value changes the
  NEFC_MAX line and nothing else; and the default capacity is still the one
  that holds every limit row and the rows of `ncon_max` contacts, worked out
  here from the model."""
  for name, task in helpers.TASKS.items():
    model = helpers.load_model(name)
    for unroll in (True, False):
      for ncon_max in (None, 3):
        plain = codegen.generate_header(model, task, ncon_max=ncon_max, unroll=unroll)
        assert plain == codegen.generate_header(model, task, ncon_max=ncon_max, unroll=unroll,
                                                nefc_max=None)
    assert codegen.model_info(model, task) == codegen.model_info(model, task, nefc_max=None)
    pairs = codegen.collision_pairs(model)
    assert codegen.capacities(model, pairs) == codegen.capacities(model, pairs, None, None)
    cut = codegen.generate_header(model, task, nefc_max=5).splitlines()
    plain = codegen.generate_header(model, task).splitlines()
    changed = [(a, b) for a, b in zip(plain, cut) if a != b]
    assert len(plain) == len(cut) and len(changed) <= 1
    assert all('NEFC_MAX = 5;' in b for _, b in changed)
    assert codegen.model_info(model, task, nefc_max=5)['nefc_max'] == 5
    # the default, independently: limits + min(rows of every pair's worst case,
    # ncon_max contacts of the widest pyramid)
    info = codegen.model_info(model, task)
    nrow = [1 if mx['dim'] == 1 else 2*(mx['dim'] - 1)
            for mx in (codegen.mix_pair(model, g1, g2) for g1, g2 in pairs)]
    nlimit = int(sum(bool(model.jnt_limited[j]) and model.jnt_type[j] in (2, 3)
                     for j in range(model.njnt)))
    assert info['nefc_max'] <= max(1, nlimit + info['ncon_max']*max(nrow + [1]))
    assert info['nefc_max'] >= max(1, nlimit + min(sum(nrow), info['ncon_max']*max(nrow + [1])))


# ---------------------------------------------------------------------------
# row capacity: `nefc_max` below what the contacts and limits need
# ---------------------------------------------------------------------------
NLIMIT_ACTIVE = 3


def _row_state(name):
  """(model, qpos, qvel) of two envs: one of the case's envs with the most
  contacts, NLIMIT_ACTIVE of its hinges pushed past their upper limit so that
  limit rows come before the contact rows; and an airborne env.  Returns also
  (active limit rows, contacts) of the first."""
  model, qpos, qvel, count = cc.states(name)
  K = max(k for n, k in cc.CASES if n == name)
  e = int(cc.envs_at(count, K)['>=K+4'][0])
  q = qpos[e].copy()
  hinges = [j for j in range(model.njnt) if model.jnt_limited[j] and model.jnt_type[j] == 3]
  for j in hinges[-NLIMIT_ACTIVE:]:
    q[model.jnt_qposadr[j]] = model.jnt_range[j][1] + 0.05
  airborne = int(np.flatnonzero(count == 0)[0])
  d = shim_runner.oracle_at(model, q, qvel[e], _ctrl(model))
  nlimit = d.nefc - sum(4 for c in range(d.ncon) if d.contact(c)['dist'] < 0)
  return model, np.array([q, qpos[airborne]]), qvel[[e, airborne]], nlimit, d.ncon


def _row_cuts(nlimit, ncon):
  """Row capacities: inside the limit rows, inside the second pyramid, one row
  short, and exactly enough (no warning)."""
  return (nlimit - 1, nlimit + 4 + 2, nlimit + 4*ncon - 1, nlimit + 4*ncon)


@pytest.mark.timeout(2400)
@pytest.mark.parametrize('name,shape,sanitizer', [
    # rows stored one to one: the planar models without the merge, the
    # several-lanes source, the humanoid
    ('cheetah', dict(unroll=True, extra=('-DDMC_NO_PLANAR_MERGE',)), 'address,undefined'),
    ('hopper', dict(unroll=False, extra=('-DDMC_NO_PLANAR_MERGE',)), 'address,undefined'),
    ('cheetah', dict(group=32), 'thread'), ('cheetah', dict(group=32), 'address,undefined'),
    ('humanoid', dict(group=128), 'thread'), ('humanoid', dict(group=128), 'address,undefined')])
def test_sources_at_row_capacity_match_the_oracle(name, shape, sanitizer, tmp_path):
  model, qpos, qvel, nlimit, ncon = _row_state(name)
  assert nlimit == NLIMIT_ACTIVE and ncon >= 4
  nenv = max(1, 64//shape['group']) if 'group' in shape else 1
  ctrl = _ctrl(model)
  pick = np.array([0, 1][:nenv])
  for cut in _row_cuts(nlimit, ncon):
    exe = shim_runner.build(model, helpers.TASKS[name], tmp_path, sanitizer=sanitizer,
                            nefc_max=cut, name='n%d' % cut, **shape)
    rows = shim_runner.run(exe, 1, qpos[pick], qvel[pick], ctrl, timeout=2000)
    shim_runner.compare(rows, [model]*nenv, qpos[pick], qvel[pick], ctrl, 1,
                        expect=dict(nefc_max=cut))
    full = cut < nlimit + 4*ncon
    assert rows[0][2][1] == cut and rows[0][2][3] == (cc.WARN_CNSTRFULL if full else 0)
    if nenv > 1:       # the env next to the full one: as next to an airborne one
      twin = shim_runner.run(exe, 1, qpos[[1, 1]], qvel[[1, 1]], ctrl, timeout=2000)
      assert np.array_equal(rows[1][1], twin[1][1]) and rows[1][2] == twin[1][2] == [0, 0, 0, 0]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('unroll', [True, False])
def test_one_lane_source_cuts_a_box_pyramid_at_row_capacity(unroll, tmp_path):
  model, task, q, v, ncon = _stacked_boxes()
  ctrl = np.zeros(model.nu)
  d = shim_runner.oracle_at(model, q[0], v[0], ctrl)
  # (the lowest box rests on the floor at distance 0: four contacts without rows)
  nrow = 4*sum(d.contact(c)['dist'] < 0 for c in range(ncon))
  assert d.nefc == nrow == 16
  for cut in (4 + 1, nrow - 1, nrow):
    exe = shim_runner.build(model, task, tmp_path, unroll=unroll, nefc_max=cut, name='n%d' % cut)
    rows = shim_runner.run(exe, 1, q, v, ctrl)
    shim_runner.compare(rows, [model], q, v, ctrl, 1, expect=dict(nefc_max=cut))
    assert rows[0][2][1] == cut
    assert rows[0][2][3] == (cc.WARN_CNSTRFULL if cut < nrow else 0)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('name,unroll', [('cheetah', True), ('hopper', False)])
def test_merged_planar_rows_at_row_capacity_stay_in_bounds(name, unroll, tmp_path):
  """The one-lane source stores the two pyramid edges along world y of a planar
  model as ONE row of twice the weight (DMC_PLANAR_MERGE), so its row capacity
  counts stored rows: a contact takes three where a tangent of its frame is
  exactly +-y and four otherwise, and a build with `nefc_max` rows keeps more
  contacts than the oracle with `nefcmax` rows.  The rule:
  CNSTRFULL exactly when a STORED row did not fit -- certainly below
  limits + 3*contacts, never from limits + 4*contacts on; stats[1] counts a
  stored merged row twice, as mj_makeConstraint would.  No oracle comparison
  where rows were dropped -- the safety half: a clean run under ASan + UBSan,
  the flag, the count, a finite state."""
  model, qpos, qvel, nlimit, ncon = _row_state(name)
  ctrl = _ctrl(model)
  for cut in (nlimit - 1, nlimit + 3 + 1, nlimit + 3 + 2, nlimit + 3*ncon - 1, nlimit + 4*ncon):
    exe = shim_runner.build(model, helpers.TASKS[name], tmp_path, unroll=unroll, nefc_max=cut,
                            name='n%d' % cut)
    rows = shim_runner.run(exe, 1, qpos[:1], qvel[:1], ctrl)
    (_, state, (got_ncon, got_nefc, _, warn)), = rows
    assert got_ncon == ncon and np.isfinite(state).all()
    assert warn == (cc.WARN_CNSTRFULL if cut < nlimit + 3*ncon else 0)
    assert got_nefc <= nlimit + 4*ncon
    if cut < nlimit + 3*ncon:
      assert cut <= got_nefc <= 2*cut
    else:       # nothing dropped: the oracle's step, with room for its rows
      shim_runner.compare(rows, [model], qpos[:1], qvel[:1], ctrl, 1, expect={})
