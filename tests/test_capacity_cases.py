"""The cases of tests/capacity_cases.py are what the capacity tests need --
checked with the oracle alone (no GPU, no kernel source)."""

import numpy as np
import pytest

import capacity_cases as cc
import helpers

_SETS = [pytest.param(name, K, False, id='%s-K%d' % (name, K)) for name, K in cc.CASES] + [
    pytest.param('humanoid', cc.DEFAULT_CAP, True, id='humanoid-default-cap')]


@pytest.mark.parametrize('name,K,default_cap', _SETS)
def test_cases_spread_bite_and_are_well_conditioned(name, K, default_cap):
  model, qpos, qvel, count = cc.default_cap_states() if default_cap else cc.states(name)
  assert len(qpos) == cc.NENV == 129
  full, capped = cc.oracle_model(model), cc.oracle_model(model, K)
  wide = cc.oracle_model(cc._widened(model))
  # a) the spread of the true count around the cap
  sizes = {k: len(v) for k, v in cc.envs_at(count, K).items()}
  if default_cap:       # the issue of this case: envs ABOVE the product's cap exist
    assert (count > K).sum() >= 4, sizes
  assert min(sizes.values()) >= 4, sizes
  assert (count == 0).sum() >= 4        # airborne twins for the neighbour checks
  for e in range(cc.NENV):
    d = cc.at(full, qpos[e], qvel[e])
    assert d.ncon == count[e] and d.warning[1] == 0
    ncon, nefc, warn, q1, v1, warning = cc.expected(capped, qpos[e], qvel[e], None)
    assert ncon == min(count[e], K)
    assert bool(warn & cc.WARN_CONTACTFULL) == (count[e] > K) and not warn & cc.WARN_CNSTRFULL
    # d) finite, no BADQACC (nor any other warning but CONTACTFULL)
    assert np.isfinite(q1).all() and np.isfinite(v1).all()
    assert not warning[[0, 2, 3, 4, 5, 6, 7]].any()
    # c) no candidate within 1e-4 of its margin; no capsule pair with crossing
    # axes among the kept contacts
    assert not cc.near_margin(cc.at(wide, qpos[e], qvel[e])), e
    assert not helpers._degenerate(cc.at(capped, qpos[e], qvel[e]), model), e
    # b) the capped step is not the uncapped one
    if count[e] > K:
      v_full = cc.expected(full, qpos[e], qvel[e], None)[4]
      assert np.abs(v1 - v_full).max() > 1e-3, (e, np.abs(v1 - v_full).max())


def test_widened_model_sees_candidates_short_of_the_margin():
  """The instrument of condition c): a capsule end 5e-5 above the floor is no
  contact of the model and one of the widened model."""
  model, qpos, qvel, count = cc.states('hopper')
  e = int(np.flatnonzero(count == 0)[0])
  full, wide = cc.oracle_model(model), cc.oracle_model(cc._widened(model))
  q = qpos[e].copy()
  lo, hi = 0.0, 2.0                        # bisect the root height to first touch
  for _ in range(60):
    mid = 0.5*(lo + hi)
    q[1] = qpos[e][1] - mid
    lo, hi = (lo, mid) if cc.at(full, q, qvel[e]).ncon else (mid, hi)
  q[1] = qpos[e][1] - lo + 5e-5
  assert cc.at(full, q, qvel[e]).ncon == 0
  assert cc.near_margin(cc.at(wide, q, qvel[e]))
  q[1] = qpos[e][1] - lo + 5e-4
  assert not cc.near_margin(cc.at(wide, q, qvel[e]))


def test_team_scene_has_the_contacts_the_caps_are_placed_around():
  import shim_runner
  m, qpos, qvel = cc.team_scene()
  d = shim_runner.oracle_at(m, qpos, qvel, np.zeros(m.nu))
  assert d.ncon == cc.TEAM_NCON and cc.TEAM_CAPS == (5, d.ncon - 1, d.ncon, d.ncon + 1)
  # contacts between the two trees exist, and sit past the smallest cap
  root = np.asarray(m.body_rootid)[np.asarray(m.geom_bodyid)]
  across = [c for c in range(d.ncon)
            if 0 not in (root[d.contact(c)['geom1']], root[d.contact(c)['geom2']])
            and root[d.contact(c)['geom1']] != root[d.contact(c)['geom2']]]
  assert across and min(across) >= cc.TEAM_CAPS[0]

