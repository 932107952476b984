"""Driver of the host shim (tests/host_shim): builds harness.cpp around a kernel
source for a model and a lane shape, runs it, and compares what it prints with
the fp64 oracle.  Shared by tests/test_kernel_sanitizers.py and
tests/test_model_params.py.  The shim is test infrastructure: the product path
cannot reach it."""

import os
import subprocess

import numpy as np

import helpers
import kat_models
import model_param_cases as mpc
from dm_control_amd import codegen
from dm_control_amd.mjcf import compiler
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, 'tests', 'host_shim')
CSRC = os.path.join(ROOT, 'dm_control_amd', 'csrc')


def case(name, nenv=None):
  """(model, task, qpos [n, nq], qvel [n, nv], steps) of `primitives`,
  `stacked_boxes`, `servo_arm` or a suite model.  nenv None: the env and the
  step count of the one-env-per-lane tests; else the nenv envs of a workgroup
  of several lanes per env (those tests bring their own step counts)."""
  n = nenv or 1
  if name == 'primitives':
    model, task, steps = compiler.from_xml_string(kat_models.PRIMITIVES), 0, 40
    q, v = np.tile(model.qpos0, (n, 1)), np.zeros((n, model.nv))
    q[:, 2], q[:, 9], q[:, 16] = 0.11, 0.2, 0.3     # stacked, in contact
  elif name == 'stacked_boxes':
    model, task, steps = compiler.from_xml_string(kat_models.STACKED_BOXES), 0, 60
    q = np.tile(model.qpos0, (n, 1))
    v = 0.3*np.random.RandomState(5).randn(n, model.nv)
    if nenv is None:
      q[0, 7 + 3:7 + 7] = [0.98, 0.05, -0.1, 0.15]     # tilt one box: edge contacts too
      q[0, 7 + 3:7 + 7] /= np.linalg.norm(q[0, 7 + 3:7 + 7])
  elif name == 'servo_arm':
    model, task, steps = compiler.from_xml_string(mpc.SERVO_ARM), 0, 60
    q = np.array([[0.35, -0.6], [-0.3, 0.9]])[:n]     # runs into the limit
    v = np.array([[1.5, -0.8], [-2.0, 0.5]])[:n]
  else:
    model, task, steps = helpers.load_model(name), helpers.TASKS[name], 25
    if nenv is None:
      q, v = helpers.initial_states(model, name, 4, seed=7)
      q, v = q[1:2], v[1:2]
    else:
      q, v = helpers.initial_states(model, name, max(n, 2), seed=7)
      q, v = q[-n:], v[-n:]
  return model, task, q, v, steps


def build(model, task, tmp_path, unroll=True, group=None, team=None, ncon_max=None,
          per_env=(), sanitizer='address,undefined', f64=True, extra=(), name='harness',
          nefc_max=None):
  """Compiles tests/host_shim/harness.cpp around the kernel source of the shape:
  one env per lane (csrc/dmc_kernels.hip; `unroll`), `group` lanes per env
  (csrc/dmc_coop.hip; 128: 64 lanes and the helper wavefront), or team mode
  (`team` lanes share the env; `ncon_max`).  sanitizer None: the plain -O2 build
  without contraction.  `nefc_max`: a row capacity below what the contacts of
  `ncon_max` need (no product build has one).  Returns the path of the program."""
  header = tmp_path/(name + '.h')
  text = codegen.generate_header(model, task, ncon_max=ncon_max, unroll=unroll, per_env=per_env,
                                 nefc_max=nefc_max)
  header.write_text(text.replace('static __device__ constexpr', 'static constexpr'))
  if group:
    shape = ['-DDMC_GROUP=%d' % min(group, 64), '-DDMC_COOP_DUO=%d' % (group == 128)]
  elif team:
    shape = ['-DDMC_TEAM=%d' % team]
  else:
    shape = ['-DDMC_LDS_BUDGET=16384']
  if sanitizer:
    mode = ['-O1', '-g', '-fsanitize=' + sanitizer] + (
        ['-fno-sanitize-recover=undefined'] if 'undefined' in sanitizer else []) + [
            '-fno-omit-frame-pointer']
  else:
    mode = ['-O2', '-ffp-contract=off']
  exe = tmp_path/name
  subprocess.check_call(
      ['g++', '-std=c++17', '-w', '-pthread'] + mode +
      (['-DDMC_REAL_IS_DOUBLE'] if f64 else []) + shape + list(extra) + [
          '-DDMC_MODEL_HEADER="%s"' % header,
          '-DDMC_KERNEL_SOURCE="%s"' % os.path.join(
              CSRC, 'dmc_coop.hip' if group else 'dmc_kernels.hip'),
          '-I', CSRC, '-I', SHIM, '-x', 'c++', os.path.join(SHIM, 'harness.cpp'),
          '-o', str(exe)])
  return str(exe)


def run(exe, steps, qpos, qvel, ctrl, blocks=None, timeout=600):
  """Steps the envs qpos[e], qvel[e] (with model-parameter block blocks[e], if
  the build reads one) under the constant control `ctrl`.  Returns the rows
  (env, state, (ncon, nefc, iters, warn)) in the order printed."""
  text = '%d 1\n' % steps
  for e in range(len(qpos)):
    values = np.concatenate([[] if blocks is None else blocks[e], qpos[e], qvel[e], ctrl])
    text += ' '.join('%.17g' % x for x in values) + '\n'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0', TSAN_OPTIONS='halt_on_error=1')
  out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=timeout)
  assert out.returncode == 0, out.stderr[-3000:]
  rows = []
  for line in out.stdout.splitlines():
    if line.startswith('STEP'):
      vals, tail = line.split('|')
      fields = vals.split()
      rows.append((int(fields[2]), np.array([float(x) for x in fields[3:]]),
                   [int(x) for x in tail.split()]))
  return rows


INIT_SENTINEL = -777.25      # what harness.cpp's init mode fills every field with
INIT_FIELDS = ('qpos', 'qvel', 'warm', 'ctrl', 'time', 'episode_return', 'taskdata',
               'modelparam')


def run_init(exe, nenv, seed, flags=0, task_param_i=0, ncon=None, timeout=300):
  """One launch of dmc_init_episode over `nenv` envs in a program made by
  `build` (its init mode: every field a heap block of exactly its size, filled
  with INIT_SENTINEL).  ncon [nenv]: the contact counts planted in the stats
  field.  Returns {field: [nenv, k]} as printed -- 17
  significant digits, so every value is the word the kernel wrote, exactly."""
  text = '%d %d %d %d\n' % (nenv, int(seed) & (2**64 - 1), flags, task_param_i)
  if ncon is not None:
    text += ' '.join('%d' % c for c in ncon) + '\n'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
  out = subprocess.run([exe, 'init'], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, env=env, timeout=timeout)
  assert out.returncode == 0, out.stderr[-3000:]
  rows = [line.split('|') for line in out.stdout.splitlines() if line.startswith('INIT')]
  assert [int(r[0].split()[1]) for r in rows] == list(range(nenv))
  fields = {}
  for i, name in enumerate(INIT_FIELDS):
    cols = [r[i].split()[2 if i == 0 else 0:] for r in rows]
    fields[name] = np.array([[float(x) for x in c] for c in cols]).reshape(nenv, -1)
  return fields


def compare_init(got, want, real_size, fields=INIT_FIELDS):
  """`got` of `run_init` (or of a device, same shapes) against a
  `device_init_model.Draw`: the envs the launch writes within the model's
  tolerance of each value (exact ones: the model rounded to `real`), everything
  else still `got['before']` (default: the sentinel) bit for bit.  Returns the
  largest error of a value whose bound is measured, not derived, per class of
  device_init_model.CPU_ROUNDING_FIGURE and in its unit, eps(real)*scale."""
  import device_init_model
  real = np.float32 if real_size == 4 else np.float64
  before = got.get('before', {})
  w = want.written
  figure = {kind: 0.0 for kind in device_init_model.KINDS}
  for name in fields:
    g = got[name]
    b = before.get(name, np.full(g.shape, INIT_SENTINEL))
    ref = getattr(want, name)
    if ref is None:           # a field this launch leaves alone
      np.testing.assert_array_equal(g, b, err_msg=name)
      continue
    ref = np.asarray(ref, np.float64).reshape(len(w), -1)
    np.testing.assert_array_equal(g[~w], b[~w], err_msg=name + ' of envs not drawn')
    tol = np.broadcast_to(device_init_model.atol(want, name, real_size), ref.shape)[w]
    rounded = ref[w].astype(real).astype(np.float64)
    np.testing.assert_array_equal(g[w][tol == 0], rounded[tol == 0], err_msg=name + ' (exact values)')
    err = np.abs(g[w] - ref[w])[tol > 0]
    assert np.all(err <= tol[tol > 0]), (name, float((err/tol[tol > 0]).max()))
    for kind in device_init_model.KINDS:
      scale = np.broadcast_to(device_init_model.scales(want, kind).get(name, np.zeros(1)),
                              ref.shape)[w]
      if w.any() and (scale > 0).any():
        figure[kind] = max(figure[kind], float((np.abs(g[w] - ref[w])[scale > 0]/
                                                (np.finfo(real).eps*scale[scale > 0])).max()))
  return figure


def oracle_at(model, qpos, qvel, ctrl, ncon_max=None, nefc_max=None):
  om = oracle.OracleModel(model)
  if ncon_max is not None:
    om.set_int('nconmax', ncon_max)
  if nefc_max is not None:
    om.set_int('nefcmax', nefc_max)
  d = oracle.OracleData(om)
  d.qpos[:] = qpos
  d.qvel[:] = qvel
  d.ctrl[:] = ctrl
  d.step1()
  return d


WARN_CONTACTFULL, WARN_CNSTRFULL = 2, 4     # csrc/dmc_args.h


def compare(rows, models, qpos, qvel, ctrl, steps, before_step=None, expect=None):
  """Steps the oracle of env e on models[e] next to `rows` and asserts the
  counters and the state of every row; before_step(d) sees the oracle of a row
  before it is stepped.  expect None: no warning bit may be set.  expect =
  dict(ncon_max=, nefc_max=): the oracle runs with these capacities, and the
  warning word must be exactly the CONTACTFULL / CNSTRFULL bits of the steps so
  far (the kernel's word is sticky) as the oracle's warning[1] / warning[2]
  counters moved in the pass that made each step's contacts and rows -- and no
  other counter of the oracle may move.  Returns (whether any step had
  constraint rows, the oracles after the last step)."""
  datas = [oracle_at(m, qpos[e], qvel[e], ctrl, **(expect or {})) for e, m in enumerate(models)]
  touched = False
  counted = [np.zeros(8, int) for _ in models]
  bits = [0]*len(models)
  for e, state, (ncon, nefc, iters, warn) in rows:
    d = datas[e]
    touched |= d.nefc > 0
    # contact and row counts as mj_makeConstraint counts them (a pyramid edge
    # pair that the planar models store as one row still counts as two)
    assert (ncon, nefc) == (d.ncon, d.nefc)
    if before_step:
      before_step(d)
    if expect is not None:
      moved = d.warning - counted[e]
      counted[e] = d.warning.copy()
      bits[e] |= (WARN_CONTACTFULL if moved[1] else 0) | (WARN_CNSTRFULL if moved[2] else 0)
      assert not d.warning[[0, 3, 4, 5, 6, 7]].any(), d.warning
    d.physics_step()
    assert warn == (0 if expect is None else bits[e]), (e, warn, bits[e])
    if expect is not None:      # (the step itself: BADQACC, BADQPOS / BADQVEL of its step1)
      assert not d.warning[[0, 3, 4, 5, 6, 7]].any(), d.warning
    nq = len(d.qpos)
    np.testing.assert_allclose(state[:nq], d.qpos, rtol=0, atol=1e-9)
    np.testing.assert_allclose(state[nq:], d.qvel, rtol=0, atol=1e-8)
  assert len(rows) == steps*len(models)
  return touched, datas


OBSERVE_FIELDS = ('qpos', 'qvel', 'obs', 'reward', 'sensordata', 'xpos', 'xmat', 'warn')


def run_observe(exe, qpos, qvel, ctrl, taskdata=None, nsub=1, task_param_i=0,
                task_param_r=0.0, layout=0, timeout=900):
  """The harness's observe mode over the envs qpos[e], qvel[e], ctrl[e],
  taskdata[e]: dmc_observe, then one dmc_step of `nsub` substeps.  Returns
  ({field: [nenv, k]} after dmc_observe, the same after dmc_step), every value
  the word the kernel wrote (17 significant digits)."""
  n = len(qpos)
  text = '%d %d %d %.17g %d\n' % (n, nsub, task_param_i, task_param_r, layout)
  for e in range(n):
    values = np.concatenate([qpos[e], qvel[e], ctrl[e], [] if taskdata is None else taskdata[e]])
    text += ' '.join('%.17g' % x for x in values) + '\n'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0')
  out = subprocess.run([exe, 'observe'], input=text, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=timeout)
  assert out.returncode == 0, out.stderr[-3000:]
  passes = []
  for tag in ('OBSERVE', 'STEPPED'):
    rows = [line.split('|') for line in out.stdout.splitlines() if line.startswith(tag + ' ')]
    assert [int(r[0].split()[1]) for r in rows] == list(range(n)), tag
    fields = {}
    for i, name in enumerate(OBSERVE_FIELDS):
      cols = [r[i].split()[2 if i == 0 else 0:] for r in rows]
      fields[name] = np.array([[float(x) for x in c] for c in cols]).reshape(n, -1)
    passes.append(fields)
  return passes[0], passes[1], out.stdout


def compare_observe(got, model, task, task_param_i, task_param_r, ctrl, taskdata, f64):
  """One pass of `run_observe` against tests/output_model.py evaluated at the
  state the pass printed, under the bounds of the device tests
  (tests/test_gpu_outputs.py): fp64 1e-9 in `helpers.rel_err` form, fp32 the
  model's per-class bound, copies of the state exact.  Touch entries: the
  observation is log1p of the sensor."""
  import output_model as M
  real = np.float64 if f64 else np.float32
  as_stored = lambda a: None if a is None else np.asarray(a, np.float64).astype(real).astype(
      np.float64)
  want = M.evaluate(model, task, task_param_i, (task_param_r,), got['qpos'], got['qvel'],
                    as_stored(ctrl), as_stored(taskdata))
  n = len(want.reward)
  assert not got['warn'].any()
  scale = M.scales(want)
  tol = {k: 1e-9*scale[k] for k in M.CLASSES + ('state',)} if f64 else M.fp32_tolerances(want)
  keep = ~M.excluded(want, tol)
  assert keep.all(), 'a case state within rounding of a margin-0 bound'
  checks = [('pos', 'xpos', got['xpos'], want.xpos.reshape(n, -1)),
            ('rot', 'xmat', got['xmat'], want.xmat.reshape(n, -1)),
            ('reward', 'reward', got['reward'], want.reward.reshape(n, 1))]
  for name, g, w, kinds in (('obs', got['obs'], want.obs, want.obs_kinds),
                            ('sensordata', got['sensordata'], want.sensordata,
                             want.sensor_kinds)):
    kinds = np.array(kinds)
    for kind in M.CLASSES + ('state',):
      if (kinds == kind).any():
        checks.append((kind, '%s.%s' % (name, kind), g[:, kinds == kind], w[:, kinds == kind]))
  for kind, name, g, w in checks:
    assert g.shape == w.shape, name
    if kind == 'state':
      np.testing.assert_array_equal(g, w, err_msg=name)
    elif f64:
      assert helpers.rel_err(g, w).max() <= 1e-9, (name, helpers.rel_err(g, w).max())
    else:
      err = np.abs(g - w).max(axis=1)/(M.EPS32*scale[kind])
      assert err.max() <= M.bound_in_eps(kind), (name, int(err.argmax()), err.max())
  touch_obs = np.array(want.obs_kinds) == 'touch'
  if touch_obs.any():
    touch = got['sensordata'][:, np.array(want.sensor_kinds) == 'touch']
    eps = np.finfo(real).eps
    np.testing.assert_allclose(got['obs'][:, touch_obs], np.log1p(touch), rtol=8*eps, atol=8*eps)
