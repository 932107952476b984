"""The fused soccer task layer without a GPU: the layout of the observation row
(`codegen.soccer_observation_layout`), what codegen accepts and refuses, the build
spec, and the TASK_SOCCER output stage of csrc/dmc_kernels.hip on the host under
sanitizers (tests/host_shim/soccer_harness.cpp, a stand-alone program), compared
with the host path word by word (tests/soccer_fused_model.py).  The MI355X
counterpart is tests/test_gpu_soccer_fused.py.
"""

import os
import subprocess

import numpy as np
import pytest

import shim_runner
import soccer_fused_model as sfm
from dm_control_amd import build
from dm_control_amd import codegen
from dm_control_amd.locomotion import soccer
from dm_control_amd.locomotion.models import soccer as scene
from dm_control_amd.mjcf import compiler


def _pitch_scene(team_size):
  geometry = soccer.PitchGeometry(
      soccer.area_to_size(soccer.MINI_FOOTBALL_MIN_AREA_PER_HUMANOID*2*team_size),
      soccer.MINI_FOOTBALL_GOAL_SIZE)
  model = compiler.from_xml_string(scene.build(
      2*team_size, with_ball=True, pitch_size=geometry.size, ball=scene.REGULATION_BALL,
      goal_size=soccer.MINI_FOOTBALL_GOAL_SIZE))
  return model, geometry


@pytest.fixture(scope='module')
def pitch_2v2():
  return _pitch_scene(2)


def _toy(**kw):
  model = compiler.from_xml_string(sfm.toy_scene_xml(**kw))
  model.soccer_pitch = sfm.TOY_PITCH
  return model


# -- layout ------------------------------------------------------------------------

@pytest.mark.parametrize('players', [2, 4, 6])
def test_layout_is_contiguous_and_sized(players):
  layout = codegen.soccer_observation_layout(players)
  at = 0
  for key, (offset, extent) in layout.items():
    assert offset == at and extent > 0, key
    at += extent
  d = 199 + 15*(players - 1)
  assert list(layout)[-1] == 'game' and layout['game'] == (players*d, 2)
  assert at == players*d + 2
  assert codegen.soccer_observation_layout(4)['game'][0] + 2 == 978
  for p in range(players):
    assert layout[(p, 'joints_pos')] == (p*d, 56)


def test_layout_refuses_odd_or_missing_teams():
  for players in (0, 1, 3):
    with pytest.raises(ValueError, match='even'):
      codegen.soccer_observation_layout(players)


def test_layout_key_order_is_the_host_paths(pitch_2v2):
  """Every player's keys, in order, are what `Task.get_observation` emits -- 2v2:
  a teammate and two opponents, whose prefixes depend on the player's team."""
  model, geometry = pitch_2v2
  rs = np.random.RandomState(0)
  qpos = np.tile(model.qpos0, (2, 1)) + 0.01*rs.randn(2, model.nq)
  qvel = rs.randn(2, model.nv)
  task = soccer.Task(2, geometry, random=0)
  task._prev_action = np.zeros((2, model.nu))     # pylint: disable=protected-access
  import types
  host = task.get_observation(types.SimpleNamespace(
      data=types.SimpleNamespace(qpos=qpos, qvel=qvel), batch_size=2))
  layout = codegen.soccer_observation_layout(4)
  for p in range(4):
    keys = [(name, extent) for (player, name), (_, extent) in (
        (k, v) for k, v in layout.items() if k != 'game') if player == p]
    assert [k for k, _ in keys] == list(host[p])
    assert [e for _, e in keys] == [int(np.asarray(host[p][k]).size//2) for k in host[p]]
  assert [n for (p, n) in list(layout)[:-1] if p == 0 and n.endswith('_ego_position')] == [
      'ball_ego_position', 'teammate_0_ego_position', 'opponent_0_ego_position',
      'opponent_1_ego_position']
  assert [n for (p, n) in list(layout)[:-1] if p == 2 and n.endswith('_ego_position')] == [
      'ball_ego_position', 'opponent_0_ego_position', 'opponent_1_ego_position',
      'teammate_0_ego_position']


def test_away_team_sees_the_arena_rotated(pitch_2v2):
  """An away player's `team_goal_*` are the away goal's features: the host row of a
  home and an away player standing at the origin with no rotation, and the boxes
  the header compiles in, are `PitchGeometry`'s to the bit."""
  model, geometry = pitch_2v2
  box = codegen.soccer_boxes(geometry.size + geometry.goal_size)
  for name, want in (('home_lo', geometry.home_goal[0]), ('home_hi', geometry.home_goal[1]),
                     ('away_lo', geometry.away_goal[0]), ('away_hi', geometry.away_goal[1]),
                     ('field_lo', geometry.field[0]), ('field_hi', geometry.field[1])):
    np.testing.assert_array_equal(box[name], want)
  qpos = np.asarray(model.qpos0, np.float64)[None].copy()
  for k in range(4):
    qpos[0, 63*k:63*k + 7] = [0, 0, 0, 1, 0, 0, 0]
  row, _ = sfm.host_row(geometry, 4, codegen.CMU_WALKER_EXTENTS, qpos,
                        np.zeros((1, model.nv)), np.zeros((1, model.nu)))
  layout = codegen.soccer_observation_layout(4)
  for s, (name, dim) in enumerate(codegen.SOCCER_ARENA):
    o, n = layout[(0, name)]
    np.testing.assert_array_equal(row[0, o:o + n], box['features'][s][:dim])
    o, n = layout[(3, name)]
    np.testing.assert_array_equal(row[0, o:o + n], box['features'][(s + 4) % 8][:dim])


# -- codegen and the build spec ------------------------------------------------------

def test_task_none_header_of_a_soccer_scene_has_no_soccer_symbol(pitch_2v2):
  model, geometry = pitch_2v2
  plain = codegen.generate_header(model, codegen.TASK_NONE, ncon_max=160, unroll=False)
  assert 'SOC_' not in plain and 'soc_' not in plain and 'DMC_TASK_SOCCER' not in plain
  model.soccer_pitch = geometry.size + geometry.goal_size
  try:
    assert codegen.generate_header(model, codegen.TASK_NONE, ncon_max=160, unroll=False) == plain
    fused = codegen.generate_header(model, codegen.TASK_SOCCER, ncon_max=160, unroll=False)
  finally:
    del model.soccer_pitch
  assert '#define DMC_TASK_SOCCER 1' in fused and 'constexpr int NOBS = 978;' in fused
  assert 'constexpr int TASK = 10;' in fused and codegen.TASK_SOCCER == 10
  assert 'constexpr int SOC_NQW = 63;' in fused and 'constexpr int SOC_NUW = 56;' in fused
  assert 'soc_qadr[] = {0, 63, 126, 189};' in fused and 'constexpr int SOC_BALL_V = 248;' in fused


def test_codegen_reads_the_extents_from_the_trees_and_refuses_other_models():
  toy = _toy()
  players, extents, ball = codegen.soccer_trees(toy)
  assert players == [(0, 0, 0), (9, 8, 2)] and extents == sfm.TOY_EXTENTS and ball == (18, 16)
  assert codegen.observation_size(toy, codegen.TASK_SOCCER) == 2*(9 - 7 + 8 - 6 + 1 + 3 + 2 + 9 + 15 + 18) + 2
  with pytest.raises(codegen.UnsupportedModelError, match='players differ'):
    codegen.generate_header(_toy(num_walkers=2, odd_walker=True), codegen.TASK_SOCCER, unroll=False)
  with pytest.raises(codegen.UnsupportedModelError, match='ball'):
    codegen.generate_header(_toy(num_walkers=3, with_ball=False), codegen.TASK_SOCCER,
                            unroll=False)
  with pytest.raises(codegen.UnsupportedModelError):
    codegen.generate_header(_toy(num_walkers=2, with_ball=False), codegen.TASK_SOCCER,
                            unroll=False)
  no_pitch = compiler.from_xml_string(sfm.toy_scene_xml())
  with pytest.raises(codegen.UnsupportedModelError, match='soccer_pitch'):
    codegen.generate_header(no_pitch, codegen.TASK_SOCCER, unroll=False)


def test_build_spec_refuses_other_shapes_and_keys_the_pitch():
  toy = _toy()
  for mode in ('coop', 'auto', 'unrolled'):
    with pytest.raises(ValueError, match='TASK_SOCCER'):
      build.spec(toy, codegen.TASK_SOCCER, 'f32', None, (), mode, None, 64)
  with pytest.raises(ValueError, match='TASK_SOCCER'):
    build.spec(toy, codegen.TASK_SOCCER, 'f32', None, (), 'rolled', None, 64, rollout=True)
  team = build.spec(toy, codegen.TASK_SOCCER, 'f32', None, (), 'team', None, 64)
  assert '-DDMC_TEAM=64' in team.flags
  rolled = build.spec(toy, codegen.TASK_SOCCER, 'f32', None, (), 'rolled', None, 64)
  assert all(t.unroll is not True for t in rolled.tiers)
  key = build.model_key(toy, codegen.TASK_SOCCER, 'f32', None, team.flags, False)
  other = _toy()
  other.soccer_pitch = (7.0,) + sfm.TOY_PITCH[1:]
  assert build.model_key(other, codegen.TASK_SOCCER, 'f32', None, team.flags, False) != key
  # a build without the task does not see the pitch
  assert (build.model_key(other, 0, 'f32', None, team.flags, False) ==
          build.model_key(toy, 0, 'f32', None, team.flags, False))


def test_load_takes_the_keyword_and_default_is_the_host_task(monkeypatch):
  """`load(fused_task=...)` up to the point where Physics would be built."""
  seen = []
  class Stop(Exception):
    pass
  def fake(*args, **kwargs):
    seen.append((args, kwargs))
    raise Stop
  monkeypatch.setattr(soccer.Physics, '__init__', fake)
  with pytest.raises(Stop):
    soccer.load(1, fused_task=True, environment_kwargs=dict(batch_size=2))
  (_, model), kwargs = seen[-1]
  assert kwargs['task'] == codegen.TASK_SOCCER and kwargs['ncon_max'] == 80
  g = soccer.PitchGeometry(soccer.area_to_size(200.0), soccer.MINI_FOOTBALL_GOAL_SIZE)
  assert model.soccer_pitch == g.size + g.goal_size
  with pytest.raises(Stop):
    soccer.load(1, environment_kwargs=dict(batch_size=2))
  assert 'task' not in seen[-1][1]
  assert issubclass(soccer.FusedTask, soccer.Task) and hasattr(soccer, 'SoccerVecEnv')


# -- the output stage on the host, under sanitizers --------------------------------

def _build_harness(tmp_path, team, sanitizer, f64=True):
  model = _toy()
  header = tmp_path/'model.h'
  text = codegen.generate_header(model, codegen.TASK_SOCCER, ncon_max=16, unroll=False)
  header.write_text(text.replace('static __device__ constexpr', 'static constexpr'))
  exe = tmp_path/'soccer_harness'
  subprocess.check_call(
      ['g++', '-std=c++17', '-w', '-pthread', '-O1', '-g', '-fsanitize=' + sanitizer,
       '-fno-omit-frame-pointer'] +
      (['-fno-sanitize-recover=undefined'] if 'undefined' in sanitizer else []) +
      (['-DDMC_REAL_IS_DOUBLE'] if f64 else []) +
      # (team mode keeps the matrices in the workspace: lower the threshold below which
      # they are per-lane arrays to under the toy scene's 22 dofs)
      (['-DDMC_TEAM=%d' % team, '-DDMC_MAT_PRIVATE_BYTES=1024'] if team > 1 else []) + [
          '-DDMC_MODEL_HEADER="%s"' % header,
          '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(shim_runner.CSRC, 'dmc_kernels.hip'),
          '-I', shim_runner.CSRC, '-I', shim_runner.SHIM, '-x', 'c++',
          os.path.join(shim_runner.SHIM, 'soccer_harness.cpp'), '-o', str(exe)])
  return model, str(exe)


def _run_harness(exe, model, qpos, qvel, stored, ctrl):
  n = len(qpos)
  text = '%d 1\n' % n
  for e in range(n):
    text += ' '.join('%.17g' % x for x in np.concatenate(
        [qpos[e], qvel[e], stored[e], ctrl[e]])) + '\n'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', TSAN_OPTIONS='halt_on_error=1')
  out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=600)
  assert out.returncode == 0, out.stderr[-3000:]
  fields = ('qpos', 'qvel', 'obs', 'reward', 'episode_return', 'ctrl', 'warn')
  passes = []
  for tag in ('OBSERVE', 'STEPPED'):
    rows = [line.split('|') for line in out.stdout.splitlines() if line.startswith(tag + ' ')]
    assert [int(r[0].split()[1]) for r in rows] == list(range(n)), tag
    got = {}
    for i, name in enumerate(fields):
      cols = [r[i].split()[2 if i == 0 else 0:] for r in rows]
      got[name] = np.array([[float(x) for x in c] for c in cols]).reshape(n, -1)
    passes.append(got)
  return passes


def _goal_cases(model, real):
  """States of the toy scene with the ball placed on detector faces, as stored in
  `real`: (qpos, qvel, [(goal code, off court)]).  "One machine step" is the next
  `real` number."""
  pitch = soccer.PitchGeometry(sfm.TOY_PITCH[:2], sfm.TOY_PITCH[2:])
  qpos0, qvel0 = sfm.seeded_states(model, 2, sfm.TOY_EXTENTS, 1, 11, pitch)
  def stored(x, toward):      # the `real` number at x, or the nearest one on the `toward` side
    r = real(x)
    if (toward > 0 and r < x) or (toward < 0 and r > x):
      r = np.nextafter(r, real(toward*np.inf))
    return float(r)
  step = lambda x, toward: float(np.nextafter(real(x), real(toward*np.inf)))
  home_lo, home_hi, _ = pitch.home_goal
  away_lo, away_hi, _ = pitch.away_goal
  flo, fhi = pitch.field
  balls = [
      # on the front face of the away goal box (its lower x bound), inside: a goal
      (stored(away_lo[0], +1), 0.3, 0.4),
      # one machine step in front of that face: no goal (and off court: past the field edge)
      (step(stored(away_lo[0], +1), -1), 0.3, 0.4),
      # on the top face of the home goal box, and one step above it
      (float(real(home_lo[0] + 0.3)), -0.2, stored(home_hi[2], -1)),
      (float(real(home_lo[0] + 0.3)), -0.2, step(stored(home_hi[2], -1), +1)),
      # on the field's edge (inside, inclusive) and one step beyond it
      (0.5, stored(fhi[1], -1), 0.3),
      (0.5, step(stored(fhi[1], -1), +1), 0.3),
      (stored(flo[0], +1), 0.1, 1.5),       # (above the home goal, whose face is here)
      # well inside
      (0.0, 0.0, 0.3)]
  n = len(balls)
  qpos, qvel = np.tile(qpos0, (n, 1)), np.tile(qvel0, (n, 1))
  qpos[:, 18:21] = balls
  return pitch, qpos, qvel


@pytest.mark.timeout(900)
@pytest.mark.parametrize('team,sanitizer', [
    (64, 'address,undefined'), (64, 'thread'), (1, 'address,undefined')])
def test_soccer_output_stage_on_the_host(team, sanitizer, tmp_path, capsys):
  """One dmc_observe and one dmc_step of the TASK_SOCCER build of a toy scene, the
  team source with 64 lanes (one thread each) and the same source with TEAM = 1:
  every index in range (ASan, every field a heap block of its size), one writer
  per word and phase (TSan), and every word of the row within its bound of the
  host path in fp64; copies, the game block and the reward exact, for balls on and
  next to the detector faces too."""
  model, exe = _build_harness(tmp_path, team, sanitizer)
  pitch, qpos, qvel = _goal_cases(model, np.float64)
  extra_q, extra_v = sfm.seeded_states(model, 2, sfm.TOY_EXTENTS, 2, 5, pitch)
  qpos, qvel = np.concatenate([qpos, extra_q]), np.concatenate([qvel, extra_v])
  n = len(qpos)
  rs = np.random.RandomState(3)
  stored, ctrl = rs.uniform(-1, 1, (n, model.nu)), rs.uniform(-1, 1, (n, model.nu))
  observed, stepped = _run_harness(exe, model, qpos, qvel, stored, ctrl)
  assert not observed['warn'].any() and not stepped['warn'].any()
  # dmc_observe: the state as given, the stored controls as prev_action
  sfm.compare(observed['obs'], observed['reward'][:, 0], pitch, 2, sfm.TOY_EXTENTS,
              observed['qpos'], observed['qvel'], stored, np.float64, 'observe')
  game = observed['obs'][:, -2:]
  np.testing.assert_array_equal(game[:8, 0], [1, 0, -1, 0, 0, 0, 0, 0])
  # (balls 0 and 1 sit where the goal's face and the field's edge differ by rounding only)
  np.testing.assert_array_equal(game[2:8, 1], [1, 1, 0, 1, 0, 0])
  np.testing.assert_array_equal(observed['episode_return'], 0)     # dmc_observe does not accumulate
  # dmc_step: the state after the step, the new controls as prev_action
  assert np.abs(stepped['qpos'] - qpos).max() > 0
  np.testing.assert_array_equal(stepped['ctrl'], ctrl)
  sfm.compare(stepped['obs'], stepped['reward'][:, 0], pitch, 2, sfm.TOY_EXTENTS,
              stepped['qpos'], stepped['qvel'], ctrl, np.float64, 'step')
  np.testing.assert_array_equal(stepped['episode_return'], stepped['reward'])
  print(capsys.readouterr().out)


# -- the code object ------------------------------------------------------------------

@pytest.mark.timeout(900)
def test_fused_1v1_team_build_cross_compiles_within_budget():
  """gfx950 code object of `soccer.load(1, fused_task=True)` (fp32, the team shape):
  the last tier ends with an "ok" verdict, i.e. within the spill budget."""
  model, geometry = _pitch_scene(1)
  model.soccer_pitch = geometry.size + geometry.goal_size
  path = build.build_model(model, codegen.TASK_SOCCER, 'f32', 80, mode='team')
  assert os.path.exists(path)
  with open(path + '.verdict') as f:
    assert f.read().split()[0] == 'ok'
