"""The selection matrix (tests/selection_matrix.py) equals the policy; the
argument sets `build_model` refuses are pinned.  No GPU."""

import pytest

import helpers
import selection_matrix as sm
from dm_control_amd import build
from dm_control_amd import suite


def test_shipped_list_equals_the_policy():
  """A policy edit (`_COOP_POLICY`, `_COOP_POLICY_F64`, `build.lds_budget_for`,
  a new domain) fails here until the new shape has its line in `SHIPPED` --
  and the GPU tests are parametrized over `SHIPPED`."""
  got = sm.enumerate_selections()
  assert set(got) == set(sm.SHIPPED), (
      'not in SHIPPED: %s; in SHIPPED only: %s' % (
          sorted(set(got) - set(sm.SHIPPED), key=str),
          sorted(set(sm.SHIPPED) - set(got), key=str)))
  assert got == sm.SHIPPED          # same order, no duplicates
  assert len({sm.line_id(line) for line in sm.SHIPPED}) == len(sm.SHIPPED)
  # the boundaries really come from the classes
  assert {1024, 2048, 4096, 8192, 16384, 32768} <= set(sm.policy_boundaries())
  for domain, precision, mode, group, lds_budget, lo, hi in sm.SHIPPED:
    assert (group is None) == (mode != 'coop')
    assert (lds_budget is None) == (mode != 'auto')
    assert hi is None or lo <= hi


def test_the_recorder_leaves_the_product_as_it_was():
  real = build.realise
  sm.select('cheetah', 'f32', 8192)
  assert build.realise is real


def test_humanoid_mixed_is_refused_by_name():
  """precision='mixed' exists for the one-env-per-lane kernel only and the
  humanoid runs on the several-lanes kernel at every batch size: the
  combination cannot be built, and says why."""
  refused = [line for line in sm.SHIPPED if line[2] == sm.REFUSED]
  assert refused == [('humanoid', 'mixed', sm.REFUSED, None, None, 1, None)]
  with pytest.raises(ValueError, match='one-env-per-lane kernel'):
    build.build_model(helpers.load_model('humanoid'), helpers.TASKS['humanoid'],
                      'mixed', mode='coop', group=128)
  for batch_size in (1, 8192, 65536):
    with pytest.raises(ValueError, match='one-env-per-lane kernel'):
      suite.load('humanoid', 'stand', environment_kwargs={
          'batch_size': batch_size, 'precision': 'mixed'})


def test_groups_whose_working_set_exceeds_lds_are_refused():
  """8 lanes per env = 8 envs per workgroup: the fp64 cheetah's working sets do
  not fit one workgroup's LDS (the static_assert of csrc/dmc_coop.hip).
  `build_model` turns the compiler's failure into a ValueError that names the
  way out; nothing is left behind that could be loaded."""
  if build.backend() != 'hipcc':
    pytest.skip('needs hipcc')
  assert sm.SMALL_GROUPS_REFUSED == (('cheetah', 8, 'f64'),)
  model = helpers.load_model('cheetah')
  for _ in range(2):      # compiled, then answered from the recorded refusal
    with pytest.raises(ValueError, match='do not fit in LDS') as info:
      build.build_model(model, helpers.TASKS['cheetah'], 'f64', mode='coop', group=8)
    assert isinstance(info.value, RuntimeError)   # also what a failed build is
  with pytest.raises(ValueError, match='group must be'):
    build.build_model(model, helpers.TASKS['cheetah'], 'f64', mode='coop', group=4)
