"""`build.spec` is pure and `build.realise` fails closed: what the ladder of
dm_control_amd/build.py returns, refuses and leaves on disk.  hipcc
cross-compiles the pendulum (seconds per build) into a temporary directory; a
tier is put over budget by giving it a budget of -1 spilled SGPRs.  No GPU."""

import os
import re
import subprocess

import pytest

import helpers
from dm_control_amd import build


def _refuse(*args, **kwargs):
  raise AssertionError('spec() must not start a process')


def test_spec_is_pure_and_resolves_the_request(monkeypatch, tmp_path):
  model = helpers.load_model('cheetah')       # 9 dofs: the "semi" tier applies
  humanoid = helpers.load_model('humanoid')   # 27 dofs: never "semi"
  monkeypatch.setattr(build, '_BUILD', str(tmp_path/'absent'))
  monkeypatch.setattr(subprocess, 'run', _refuse)
  monkeypatch.setattr(subprocess, 'check_call', _refuse)
  monkeypatch.delenv('DMC_ROLLED_STRICT', raising=False)
  monkeypatch.setenv('DMC_EXTRA_FLAGS', '-DX=1')
  unrolled, semi, rolled = build._UNROLLED, build._SEMI, build._ROLLED
  s = build.spec(model, 2, 'f64', None, (), 'coop', 36*1024, 128)
  assert (s.source, s.real, s.tiers) == ('dmc_coop.hip', 'f64', (build._COOP,))
  assert s.flags == ('-DDMC_GROUP=64', '-DDMC_COOP_DUO=1')    # no -DDMC_LDS_BUDGET
  assert (s.model, s.task, s.ncon_max) == (model, 2, None)
  assert (s.precision, s.mode, s.group, s.lds_budget) == ('f64', 'coop', 128, 36*1024)
  s = build.spec(model, 0, 'f32', 64, (), 'team', None, 64)
  assert (s.source, s.real, s.tiers) == ('dmc_kernels.hip', 'f32', (semi, rolled))
  assert (s.flags, s.mode, s.ncon_max) == (('-DDMC_TEAM=64',), 'team', 64)
  s = build.spec(model, 2, 'mixed', None, None, 'auto', 64*1024, 64)
  assert (s.precision, s.real, s.tiers) == ('mixed', 'f32', (unrolled, semi, rolled))
  assert s.flags == ('-DX=1', '-DDMC_STATE_COMP=1', '-DDMC_LDS_BUDGET=65536')
  s = build.spec(model, 2, 'f32', None, (), 'auto', 128*1024, 64)
  assert (s.flags, s.tiers) == ((), (unrolled, semi, rolled))
  assert build.spec(model, 2, 'f32', None, (), 'unrolled', None, 64).tiers == (unrolled,)
  monkeypatch.setenv('DMC_ROLLED_STRICT', '1')
  assert build.spec(model, 2, 'f32', None, (), 'rolled', None, 64).tiers == (rolled,)
  assert (model.nv, humanoid.nv) == (9, 27)
  assert build.spec(humanoid, 3, 'f32', None, (), 'auto', None, 64).tiers == (unrolled, rolled)
  for args, message in (
      (('f16', None, (), 'auto', None, 64), 'precision must be'),
      (('f32', None, (), 'fast', None, 64), 'mode must be'),
      (('mixed', None, (), 'coop', None, 64), 'one-env-per-lane kernel'),
      (('mixed', None, (), 'team', None, 64), 'one-env-per-lane kernel'),
      (('f32', None, (), 'coop', None, 4), 'group must be')):
    with pytest.raises(ValueError, match=message):
      build.spec(model, 2, *args)
  assert not os.path.exists(build._BUILD)


@pytest.fixture
def ladder(monkeypatch, tmp_path):
  """The pendulum, an empty build directory, and the log of compiles."""
  if build.backend() != 'hipcc':
    pytest.skip('needs hipcc')
  monkeypatch.setattr(build, '_BUILD', str(tmp_path/'_build'))
  monkeypatch.setenv('DMC_BUILD_LOG', str(tmp_path/'compiles.log'))
  monkeypatch.delenv('DMC_ALLOW_OVERBUDGET', raising=False)
  monkeypatch.delenv('DMC_ROLLED_STRICT', raising=False)

  def compiles():
    if not os.path.exists(str(tmp_path/'compiles.log')):
      return []
    with open(str(tmp_path/'compiles.log')) as f:
      return [line.split('unroll=')[1].split()[0] for line in f]

  def loadable():
    return sorted(n for n in os.listdir(build._BUILD) if not n.endswith(('.h', '.verdict')))
  return helpers.load_model('pendulum'), helpers.TASKS['pendulum'], compiles, loadable


def _over(monkeypatch, *names):
  for name in names:
    monkeypatch.setattr(build, name, getattr(build, name)._replace(max_sgpr=-1))


@pytest.mark.parametrize('mode,tiers,message', [
    ('unrolled', ('_UNROLLED',), 'the unrolled build of this model spills'),
    ('coop', ('_COOP',), 'the several-lanes build of this model spills'),
    ('rolled', ('_SEMI', '_ROLLED'), 'the rolled build of this model spills')])
def test_over_budget_builds_only_under_the_override(ladder, monkeypatch, mode, tiers,
                                                    message):
  """Beyond the budget the last tier raises and leaves nothing loadable; under
  `allow_overbudget()` it builds and records; afterwards the record answers,
  without compiling, and still refuses without the override."""
  model, task, compiles, loadable = ladder
  _over(monkeypatch, *tiers)
  with pytest.raises(RuntimeError, match=message):
    build.build_model(model, task, 'f32', mode=mode)
  assert loadable() == [] and len(compiles()) == len(tiers)
  with build.allow_overbudget():
    path = build.build_model(model, task, 'f32', mode=mode)
    assert loadable() == [os.path.basename(path)]
    ncompiled = len(compiles())
    assert ncompiled == len(tiers) + 1        # the last tier only, once more
    assert build.build_model(model, task, 'f32', mode=mode) == path
  with pytest.raises(RuntimeError, match=message) as info:
    build.build_model(model, task, 'f32', mode=mode)
  assert re.search(r'spills \(\d+, \d+\) \(VGPR, SGPR\)', str(info.value))   # from the record
  assert len(compiles()) == ncompiled


def test_auto_never_returns_a_build_made_under_the_override(ladder, monkeypatch):
  model, task, compiles, loadable = ladder
  _over(monkeypatch, '_UNROLLED')
  with build.allow_overbudget():
    over = build.build_model(model, task, 'f32', mode='unrolled')
    assert loadable() == [os.path.basename(over)]
    auto = build.build_model(model, task, 'f32')
  assert auto != over and compiles() == ['True', "'semi'"]
  assert build.build_model(model, task, 'f32') == auto
  assert build.build_model(model, task, 'f32', mode='rolled') == auto
  assert compiles() == ['True', "'semi'"]
  # force: the tier `auto` selects is compiled again -- "semi" is not skipped
  assert build.build_model(model, task, 'f32', force=True) == auto
  assert compiles() == ['True', "'semi'", 'True', "'semi'"]
  # a code object without a record is not trusted: compiled again
  os.remove(auto + '.verdict')
  assert build.build_model(model, task, 'f32') == auto
  assert compiles()[4:] == ["'semi'"]


def test_auto_returns_the_unrolled_build_within_budget(ladder):
  model, task, compiles, loadable = ladder
  path = build.build_model(model, task, 'f32')
  assert build.build_model(model, task, 'f32', mode='unrolled') == path
  assert compiles() == ['True'] and loadable() == [os.path.basename(path)]
  with open(path + '.verdict') as f:
    assert f.read().startswith('ok (')
