"""Per-env episodes of the kernel sources (DMC_FLAG_MASKED, DMC_FLAG_EPISODES of
csrc/dmc_args.h) on the host: tests/host_shim/episode_harness.cpp is built
around a kernel source as a stand-alone program under ASan + UBSan (the
several-lanes sources under ThreadSanitizer too), run directly, and what it
prints is compared
  * for dmc_init_episode, with tests/device_init_model.py restricted to the mask;
  * for dmc_step, word by word with the env's contents before the launch (an env
    outside the mask, a finished env), with the same program's launch without a
    mask, and through shim_runner.compare with the fp64 oracle.
Every run has a timeout: a lane that waits at a barrier for one that left the
kernel hangs the program.  The MI355X counterpart is tests/test_gpu_episodes.py.
"""

import os
import re
import subprocess

import numpy as np
import pytest

import device_init_model as dim
import helpers
import shim_runner
from dm_control_amd import codegen

ARGS_H = os.path.join(shim_runner.CSRC, 'dmc_args.h')
with open(ARGS_H) as _f:
  FLAG = {n: int(v) for n, v in re.findall(r'#define\s+DMC_FLAG_(\w+)\s+(\d+)\b', _f.read())}
INT_SENTINEL = 7777          # what the harness fills the episode block with in init mode
RUN_TIMEOUT = 300


def build(model, task, tmp_path, group=None, sanitizer='address,undefined', f64=True,
          extra=()):
  """shim_runner.build with tests/host_shim/episode_harness.cpp as the program."""
  header = tmp_path/'model.h'
  text = codegen.generate_header(model, task, unroll=True)
  header.write_text(text.replace('static __device__ constexpr', 'static constexpr'))
  if group:
    shape = ['-DDMC_GROUP=%d' % min(group, 64), '-DDMC_COOP_DUO=%d' % (group == 128)]
  else:
    shape = ['-DDMC_LDS_BUDGET=16384']
  mode = ['-O1', '-g', '-fsanitize=' + sanitizer] + (
      ['-fno-sanitize-recover=undefined'] if 'undefined' in sanitizer else []) + [
          '-fno-omit-frame-pointer']
  exe = tmp_path/'episode_harness'
  subprocess.check_call(
      ['g++', '-std=c++17', '-w', '-pthread'] + mode +
      (['-DDMC_REAL_IS_DOUBLE'] if f64 else []) + shape + list(extra) + [
          '-DDMC_MODEL_HEADER="%s"' % header,
          '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(
              shim_runner.CSRC, 'dmc_coop.hip' if group else 'dmc_kernels.hip'),
          '-I', shim_runner.CSRC, '-I', shim_runner.SHIM, '-x', 'c++',
          os.path.join(shim_runner.SHIM, 'episode_harness.cpp'), '-o', str(exe)])
  return str(exe)


@pytest.fixture(scope='module')
def exe_of(tmp_path_factory):
  """The program once per (domain, lanes per env or None, f64, sanitizer)."""
  made = {}

  def get(domain, group=None, f64=True, sanitizer='address,undefined'):
    key = (domain, group, f64, sanitizer)
    if key not in made:
      model = dim.case_model(domain, None)
      # a one-lane build that steps: the transposed observation store is under test
      extra = () if group or domain not in ('cheetah', 'hopper') else ('-DEPISODE_EXPECT_OBS_STAGE=1',)
      made[key] = (model, build(model, helpers.TASKS[domain], tmp_path_factory.mktemp('episodes'),
                                group=group, f64=f64, sanitizer=sanitizer, extra=extra))
    return made[key]
  return get


def _run(exe, mode, text):
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', TSAN_OPTIONS='halt_on_error=1')
  out = subprocess.run([exe, mode], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=RUN_TIMEOUT)
  assert out.returncode == 0, out.stderr[-3000:]
  return out.stdout.splitlines()


# ---------------------------------------------------------------------------
# dmc_init_episode under a mask
# ---------------------------------------------------------------------------
def run_init(exe, nenv, seed, flags, task_param_i, mask, ncon=None):
  """{field: [nenv, k]} in shim_runner.run_init's form, plus 'episode' [nenv, 3]:
  ep_step, ep_done and the warning mask after the launch."""
  ncon = np.zeros(nenv, int) if ncon is None else ncon
  text = '%d %d %d %d\n' % (nenv, int(seed) & (2**64 - 1), flags, task_param_i)
  text += ''.join('%d %d\n' % (c, m) for c, m in zip(ncon, mask))
  rows = [line.split('|') for line in _run(exe, 'init', text) if line.startswith('INIT')]
  assert [int(r[0].split()[1]) for r in rows] == list(range(nenv))
  fields = {}
  for i, name in enumerate(shim_runner.INIT_FIELDS):
    cols = [r[i].split()[2 if i == 0 else 0:] for r in rows]
    fields[name] = np.array([[float(x) for x in c] for c in cols]).reshape(nenv, -1)
  fields['episode'] = np.array([[int(x) for x in r[8].split()] for r in rows])
  return fields


NENV = 67
MASKS = {'some': [0, 63, 64, 66], 'none': [], 'all': list(range(NENV))}
# (case of device_init_model.CASES, lanes per env of the source: None = one lane,
# fields [k][env]; 64 = several lanes, fields [env][k]).  The humanoid has no
# one-lane build; its launch is the rejection round's, ONLY_COLLIDING and mask.
INIT_CASES = [('cheetah_run', None), ('cheetah_run', 64), ('cartpole_swingup', None),
              ('cartpole_swingup', 64), ('point_mass_hard', None), ('point_mass_hard', 64),
              ('reacher_hard', None), ('reacher_hard', 64), ('humanoid_stand', 64)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize('label,group', INIT_CASES)
def test_masked_init_draws_the_model_inside_the_mask_only(label, group, exe_of):
  _, domain, poles, param = next(c for c in dim.CASES if c[0] == label)
  assert poles in (None, 1)
  f64 = group is None                 # (both precisions get a turn)
  model, exe = exe_of(domain, group, f64)
  task = helpers.TASKS[domain]
  flags, ncon = FLAG['MASKED'] | FLAG['EPISODES'], None
  if domain == 'humanoid':
    flags |= FLAG['ONLY_COLLIDING']
    ncon = np.arange(NENV) % 2 * 3          # odd envs collide: 63 is in the mask, 0, 64, 66 are clean
  seed = dim.SEEDS[1]
  got = {}
  for name, envs in MASKS.items():
    mask = np.zeros(NENV, bool)
    mask[envs] = True
    got[name] = run_init(exe, NENV, seed, flags, param, mask, ncon)
    want = dim.draw(model, task, param, seed, NENV, flags & FLAG['ONLY_COLLIDING'], ncon)
    want.written &= mask
    shim_runner.compare_init(got[name], want, 8 if f64 else 4)
    # step count, done word and warning mask: 0 where the launch wrote, else untouched
    np.testing.assert_array_equal(
        got[name]['episode'], np.where(want.written[:, None], 0, INT_SENTINEL)*np.ones((1, 3), int))
    if name == 'none':
      assert all((got[name][f] == shim_runner.INIT_SENTINEL).all() for f in shim_runner.INIT_FIELDS)
  # the full mask is the launch without one, bit for bit
  plain = run_init(exe, NENV, seed, flags & ~FLAG['MASKED'], param, np.zeros(NENV, bool), ncon)
  for f in plain:
    np.testing.assert_array_equal(got['all'][f], plain[f], err_msg=f)
  # and without DMC_FLAG_EPISODES the episode block and the warning mask stay
  bare = run_init(exe, NENV, seed, FLAG['MASKED'], param, np.ones(NENV, bool), ncon)
  assert (bare['episode'] == INT_SENTINEL).all()


# ---------------------------------------------------------------------------
# dmc_step under a mask / with episode bookkeeping
# ---------------------------------------------------------------------------
def run_step(exe, steps, flags, step_limit, mask, ep_step, ep_done, qpos, qvel, ctrl):
  """-> {t: [(rows of shim_runner.run's form, (ep_step, ep_done), every word as text)
  per env]}, t = -1: before the first launch."""
  n = len(qpos)
  text = '%d %d 1 %d %d\n' % (n, steps, flags, step_limit)
  for e in range(n):
    text += '%d %d %d ' % (mask[e], ep_step[e], ep_done[e])
    text += ' '.join('%.17g' % x for x in np.concatenate([qpos[e], qvel[e], ctrl])) + '\n'
  out = {}
  for line in _run(exe, 'step', text):
    if line.startswith('STEP'):
      head, counters, episode, words = line.split('|')
      f = head.split()
      out.setdefault(int(f[1]), []).append((
          (int(f[2]), np.array([float(x) for x in f[3:]]), [int(x) for x in counters.split()]),
          tuple(int(x) for x in episode.split()), words.strip()))
  assert sorted(out) == list(range(-1, steps)) and all(len(v) == n for v in out.values())
  return out


def _masked_step_checks(model, exe, q, v, mask, steps):
  """The two checks of a masked launch sequence: envs outside the mask keep every
  word, envs inside equal the launch without a mask bit for bit and the oracle
  within shim_runner.compare's tolerances."""
  n = len(q)
  ctrl = np.zeros(model.nu)
  zeros = np.zeros(n, int)
  masked = run_step(exe, steps, FLAG['MASKED'], 0, mask, zeros, zeros, q, v, ctrl)
  plain = run_step(exe, steps, 0, 0, zeros, zeros, zeros, q, v, ctrl)
  inside = [e for e in range(n) if mask[e]]
  assert 0 < len(inside) < n
  for t in range(steps):
    for e in range(n):
      if mask[e]:
        assert masked[t][e][2] == plain[t][e][2], (t, e)
        assert masked[t][e][2] != masked[t - 1][e][2]
      else:
        assert masked[t][e][2] == masked[-1][e][2], (t, e)
  rows = [(inside.index(row[0]), row[1], row[2])
          for t in range(steps) for row, _, _ in masked[t] if mask[row[0]]]
  shim_runner.compare(rows, [model]*len(inside), q[inside], v[inside], ctrl, steps)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('domain', ['cheetah', 'hopper'])
def test_masked_step_one_lane_source(domain, exe_of):
  """Three lanes of one workgroup, the middle one outside the mask, observations
  in the agent layout: the harness asserts at compile time that this build
  transposes them through LDS (OBS_STAGE_FITS), the store that assumed "lanes
  0..nvalid-1 are exactly the active ones"."""
  model, exe = exe_of(domain)
  q, v = helpers.initial_states(model, domain, 3, seed=7)
  _masked_step_checks(model, exe, q, v, [1, 0, 1], steps=6)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('group,sanitizer', [
    (32, 'address,undefined'), (32, 'thread'), (128, 'address,undefined'), (128, 'thread')])
def test_masked_step_several_lanes_source(group, sanitizer, exe_of):
  """hopper, 32 lanes per env: the two envs of a wavefront, one outside the mask;
  128 lanes: two workgroups (both wavefronts of the masked-out env leave)."""
  model, exe = exe_of('hopper', group, True, sanitizer)
  q, v = helpers.initial_states(model, 'hopper', 2, seed=7)
  _masked_step_checks(model, exe, q, v, [0, 1] if group == 32 else [1, 0], steps=3)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('domain,group', [('cheetah', None), ('hopper', 32)])
def test_episode_bookkeeping(domain, group, exe_of):
  """DMC_FLAG_EPISODES, step limit 3, env 1 two steps into its episode, a NaN in
  env 2's qvel: step counts, bit 0 exactly at the limit, bit 1 for the bad env
  alone, and a finished env frozen word for word."""
  model, exe = exe_of(domain, group)
  n = 3 if group is None else 4
  q, v = helpers.initial_states(model, domain, n, seed=7)
  v[2, 0] = np.nan
  zeros = np.zeros(n, int)
  start = np.array([0, 2, 0, 0][:n])
  out = run_step(exe, 4, FLAG['EPISODES'], 3, zeros, start, zeros, q, v, np.zeros(model.nu))
  episode = np.array([[row[1] for row in out[t]] for t in range(4)])      # [t, env, (step, done)]
  want_steps = np.array([[1, 3, 1, 1], [2, 3, 1, 2], [3, 3, 1, 3], [3, 3, 1, 3]])[:, :n]
  want_done = np.array([[0, 1, 2, 0], [0, 1, 2, 0], [1, 1, 2, 1], [1, 1, 2, 1]])[:, :n]
  np.testing.assert_array_equal(episode[:, :, 0], want_steps)
  np.testing.assert_array_equal(episode[:, :, 1], want_done)
  for t in range(1, 4):
    for e in range(n):
      frozen = want_done[t - 1, e] != 0
      assert (out[t][e][2] == out[t - 1][e][2]) == frozen, (t, e)
  # the bad env was put back to qpos0 (mj_checkPos) and says why; the others say nothing
  warn = [row[0][2][3] for row in out[0]]
  assert warn[2] != 0 and not any(w for e, w in enumerate(warn) if e != 2)
  # a settle launch (no outputs) neither counts nor freezes
  settle = run_step(exe, 1, FLAG['EPISODES'] | FLAG['NO_OUTPUT'], 3, zeros, start,
                    np.array([0, 1, 0, 0][:n]), q, np.nan_to_num(v), np.zeros(model.nu))
  assert [row[1] for row in settle[0]] == [row[1] for row in settle[-1]]
  assert settle[0][1][2] != settle[-1][1][2]
  # DMC_FLAG_ZERO_TIME: the stepped envs end at time 0, the masked-out one keeps its clock
  zt = run_step(exe, 1, FLAG['ZERO_TIME'] | FLAG['NO_OUTPUT'] | FLAG['MASKED'], 0,
                np.array([1, 0, 1, 1][:n]), zeros, zeros, q, np.nan_to_num(v), np.zeros(model.nu))
  assert zt[0][1][2] == zt[-1][1][2] and zt[0][0][2] != zt[-1][0][2]
  plain = run_step(exe, 1, FLAG['NO_OUTPUT'], 0, zeros, zeros, zeros, q, np.nan_to_num(v),
                   np.zeros(model.nu))
  nq, nv = model.nq, model.nv
  time_at = nq + 2*nv                # the words of an env: qpos, qvel, warm start, time, ...
  for e in (0, 2):
    a, b = zt[0][e][2].split(), plain[0][e][2].split()
    assert float(a[time_at]) == 0 and float(b[time_at]) == model.opt.timestep
    assert a[:time_at] == b[:time_at] and a[time_at + 1:] == b[time_at + 1:]
