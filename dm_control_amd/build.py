"""hipcc driver: builds libdmc_hip.so and per-model gfx950 code objects.

Everything is built IN-TREE (csrc/libdmc_hip.so, csrc/_build/<key>.hsaco) so
the artefacts travel to the GPU box with the repository snapshot.  hipcc
cross-compiles for gfx950 without a GPU present.

`build_model(...)` is `realise(spec(...))`.  `spec` checks the arguments and
resolves them, touching no file, into source, compile precision, -D flags and
the tiers the request may use; `_flags` alone writes the compiler's command line.
The ladder: unrolled, "semi" (generic source, backend unroller on; small models)
and strictly rolled for "auto", the last two for "rolled" / "team", the first
for "unrolled"; "coop" is one tier on csrc/dmc_coop.hip.  Each code object has
one sidecar record, `<key>.hsaco.verdict`: "ok", "over" (budget) or "nolds" (does
not fit in LDS), with the spill counts.  `realise` takes a tier's verdict from
the record, or compiles to `.tmp`, records, and only then publishes
(os.replace); it returns the first "ok" tier, falls through, raises at the
last.  "over" is returned only as the last tier of a request made under
`allow_overbudget()`; a file without a record never is.
"""

import collections
import contextlib
import hashlib
import os
import shutil
import subprocess

from dm_control_amd import codegen

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
_BUILD = os.path.join(_CSRC, '_build')
LIB_PATH = os.path.join(_CSRC, 'libdmc_hip.so')
ARCH = 'gfx950'


def _hipcc():
  exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
  if not os.path.exists(exe):
    raise RuntimeError('hipcc not found; cannot build the HIP extension')
  return exe


def backend():
  """How model code objects are built: "hipcc" (the toolchain's driver, what
  `__graft_entry__.build()` uses ahead of time) or "hiprtc" -- in-process
  through `dmc_model_compile` of the C ABI (HIP runtime compilation: needs the
  ROCm runtime only, no hipcc executable).  `$DMC_BUILD_BACKEND` selects;
  default: hipcc when it exists, else hiprtc."""
  choice = os.environ.get('DMC_BUILD_BACKEND')
  if choice in ('hipcc', 'hiprtc'):
    return choice
  exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
  return 'hipcc' if os.path.exists(exe) else 'hiprtc'


def _newer(target, sources):
  if not os.path.exists(target):
    return False
  t = os.path.getmtime(target)
  return all(os.path.getmtime(s) <= t for s in sources)


def build_library(force=False):
  """Compiles the C-ABI runtime (include/dmc_hip.h) into libdmc_hip.so."""
  srcs = [os.path.join(_CSRC, 'dmc_api.cpp'),
          os.path.join(_CSRC, 'dmc_args.h'),
          os.path.join(_CSRC, 'dmc_launch.h'),
          os.path.join(_CSRC, '..', '..', 'include', 'dmc_hip.h')]
  if not force and _newer(LIB_PATH, srcs):
    return LIB_PATH
  cmd = [_hipcc(), '-O2', '-fPIC', '-shared', '-std=c++17',
         '--offload-arch=' + ARCH, '-o', LIB_PATH, srcs[0]]
  subprocess.check_call(cmd)
  return LIB_PATH


# Spill budget of the fully unrolled ("static") build.  Kernels far beyond it
# (fp64 builds of 20-dof models: ~1900 VGPR + ~200 SGPR spills, 300 KB of code)
# have produced wrong results on gfx950 with ROCm 7.2 while the same source is
# correct on the host under ASan/UBSan and with gcc/clang -O3 (see DESIGN.md,
# "compiler hazard"), so `mode="auto"` falls back to the rolled build, whose
# per-lane arrays are explicit scratch objects instead of register spills.
MAX_VGPR_SPILLS = 128
MAX_SGPR_SPILLS = 128
# The several-lanes kernel (csrc/dmc_coop.hip) keeps per-env data in LDS and its
# uniform address arithmetic in SGPRs: every suite build spills 136-386 SGPRs
# (to VGPR lanes, no scratch traffic) and at most 7 VGPRs, and every one that
# `Physics` can select is parity-tested per step against the oracle
# (tests/selection_matrix.py lists them; a CPU test keeps the list equal to the
# policy, tests/test_gpu_selection.py runs each line).  What the guard must refuse there
# is the same thing as above: builds that spill VGPRs wholesale to scratch
# (the 62-dof soccer walker: 1652 fp32 / 6552 fp64).
COOP_MAX_SGPR_SPILLS = 640
SEMI_ROLLED_MAX_NV = 16     # see _SEMI: the generic tier with the backend unroller on


# fp32 builds: v_rcp / v_rsq based division and sqrt (<= 2.5 ulp) instead of the
# IEEE sequences, and x / y as x * rcp(y).  Without the second flag LLVM lowers
# every fp32 division to a frexp / rcp / ldexp sequence of 8 instructions -- 9 %
# of the cheetah kernel's code; with it the step takes 5 % (cheetah) to 10 %
# (humanoid) less time.  The fp64 build keeps exact division.
_FP32_FLAGS = ('-fno-hip-fp32-correctly-rounded-divide-sqrt', '-freciprocal-math')


# "rolled" has to mean rolled: the AMDGPU backend raises the unroll thresholds
# of loops that index private arrays (to promote them to registers), which
# turned the generic loops of mid-size models back into straight-line code --
# the rolled fp64 build of the 62-dof walker spilled 14591 VGPRs, took 68 s to
# compile and returned a wrong mass-matrix factor on the GPU (round 3).  With
# the loop unroller off the same build spills nothing and compiles in 5 s.
_ROLLED_FLAGS = ('-fno-unroll-loops',)


def model_key(model, task, precision, ncon_max=None, extra_flags=(),
              unroll=True, per_env=()):
  src = os.path.join(_CSRC, 'dmc_kernels.hip')
  h = hashlib.sha1()
  h.update(model.content_hash().encode())
  h.update(('%d/%s/%r/%r/%s/%d/%s/%s' % (
      task, precision, ncon_max, tuple(extra_flags),
      os.environ.get('DMC_PRAGMA_UNROLL_THRESHOLD', ''), int(unroll is True),
      ' '.join(_FP32_FLAGS),
      '' if unroll is True else ('semi' if unroll == 'semi' else ' '.join(_ROLLED_FLAGS)))).encode())
  if per_env:       # (nothing added for (): the key of a build without per-env fields)
    h.update(('/per_env=' + ','.join(per_env)).encode())
  if task == codegen.TASK_SOCCER:   # the pitch is compiled in and is not a model field
    h.update(('/soccer_pitch=%r' % (codegen.soccer_pitch_of(model),)).encode())
  for path in (src, os.path.join(_CSRC, 'dmc_coop.hip'),
               os.path.join(_CSRC, 'dmc_args.h'), codegen.__file__):
    with open(path, 'rb') as f:
      h.update(f.read())
  return h.hexdigest()[:20]


def _spills(remarks, kernel='dmc_step'):
  """(vgpr, sgpr) spill counts of `kernel` from -Rpass-analysis remarks, or
  None if the remarks do not hold them (the caller then treats the build as
  over budget: the guard fails closed)."""
  vg = sg = None
  inside = False
  for line in remarks.splitlines():
    if 'Function Name:' in line:
      inside = ('Function Name: %s ' % kernel) in line + ' '
    elif inside and 'VGPRs Spill:' in line:
      vg = int(line.split('VGPRs Spill:')[1].split()[0])
    elif inside and 'SGPRs Spill:' in line:
      sg = int(line.split('SGPRs Spill:')[1].split()[0])
  if vg is None or sg is None:
    return None
  return vg, sg


_OVERBUDGET_MSG = (
    'the unrolled build of this model spills %%s (VGPR, SGPR) registers, beyond '
    'the budget of %d / %d within which this kind of build is trusted '
    '(DESIGN.md 3.4: an over-budget build has produced wrong results on '
    'gfx950); use mode="auto" / "rolled" / "coop", or set '
    '$DMC_ALLOW_OVERBUDGET=1 to build it anyway' % (MAX_VGPR_SPILLS, MAX_SGPR_SPILLS))


_COOP_OVERBUDGET_MSG = (
    'the several-lanes build of this model spills %%s (VGPR, SGPR) registers '
    '(budget %d / %d); set $DMC_ALLOW_OVERBUDGET=1 to build it anyway'
    % (MAX_VGPR_SPILLS, COOP_MAX_SGPR_SPILLS))

_ROLLED_OVERBUDGET_MSG = (
    'the rolled build of this model spills %%s (VGPR, SGPR) registers (budget '
    '%d / %d); set $DMC_ALLOW_OVERBUDGET=1 to build it anyway'
    % (MAX_VGPR_SPILLS, COOP_MAX_SGPR_SPILLS))


class LdsWorkingSetError(ValueError, RuntimeError):
  """`group` lanes per env put 64/group envs into one workgroup's LDS; this
  model's working set times that many envs does not fit (the static_assert of
  csrc/dmc_coop.hip).  A ValueError: the argument set cannot be built."""


_LDS_MSG = ('%d lanes per env (%s): the working sets of the %d envs of a workgroup '
            'do not fit in LDS; use a larger group or the one-env-per-lane kernel')


def _allow_overbudget():
  """Explicit override for experiments and the canary test."""
  return os.environ.get('DMC_ALLOW_OVERBUDGET') == '1'


@contextlib.contextmanager
def allow_overbudget():
  """`with build.allow_overbudget():` -- builds inside may exceed the spill
  budget (the canary test and tools/spill_hazard/ only; never the product)."""
  prev = os.environ.get('DMC_ALLOW_OVERBUDGET')
  os.environ['DMC_ALLOW_OVERBUDGET'] = '1'
  try:
    yield
  finally:
    if prev is None:
      del os.environ['DMC_ALLOW_OVERBUDGET']
    else:
      os.environ['DMC_ALLOW_OVERBUDGET'] = prev


def _within_spill_budget(spills, max_sgpr):
  return (spills is not None and spills[0] <= MAX_VGPR_SPILLS
          and spills[1] <= max_sgpr)


# One tier: `unroll` as model_key takes it (True: the unrolled source; "semi" /
# False: the generic one), the SGPR spill budget within which it is trusted,
# and what it says beyond that budget as the last tier of a request.
Tier = collections.namedtuple('Tier', 'unroll max_sgpr refusal')
_UNROLLED = Tier(True, MAX_SGPR_SPILLS, _OVERBUDGET_MSG)
# Generic ("rolled") source, two tiers.  First with the backend's loop unroller
# left on: for small models it turns the per-lane loops back into mostly
# straight-line code within the spill budget (cheetah fp64: 14 VGPR / 300 SGPR
# spills, 0.33 ms per launch against 1.33 ms strictly rolled).  Beyond the
# budget -- mid-size models: humanoid fp64 3644, the 62-dof walker 14591 spilled
# VGPRs -- the strictly rolled form (-fno-unroll-loops: no spills at all).
# Only small models take the first: it is the regime every GPU parity test of
# a suite fp64 build covers, and the one time the unroller was let loose on a
# big model (the 2v2 pitch) it produced wrong code (csrc/dmc_kernels.hip,
# DMC_KEEP_ROLLED).
_SEMI = Tier('semi', COOP_MAX_SGPR_SPILLS, None)
_ROLLED = Tier(False, COOP_MAX_SGPR_SPILLS, _ROLLED_OVERBUDGET_MSG)
# the several-lanes kernel keeps its working set in LDS; a build that spills
# beyond the budget is as untrusted as an over-budget unrolled one
_COOP = Tier(True, COOP_MAX_SGPR_SPILLS, _COOP_OVERBUDGET_MSG)

# What `build_model` was asked (model .. lds_budget, as given) and what that
# means: source file, compile precision, final -D flags, tiers in order.
Spec = collections.namedtuple(
    'Spec', 'model task ncon_max precision mode group lds_budget source real flags tiers '
            'per_env')


def spec(model, task, precision, ncon_max, extra_flags, mode, lds_budget, group,
         per_env=(), rollout=False, population=False):
  """Checks the arguments of `build_model` and resolves them into a `Spec`.
  Pure: reads the environment, touches no file and starts no process.
  `per_env`: model fields the kernels read per env (codegen.PER_ENV_FIELDS).
  `rollout`: the rollout variant of the one-env-per-lane kernel (-DDMC_ROLLOUT=1).
  `population`: the rollout variant whose policy evaluator reads its weights per
  lane, one policy per group of envs (-DDMC_POLICY_POPULATION=1)."""
  if population and not rollout:
    raise ValueError('population=True is a variant of the rollout build: it needs '
                     'rollout=True')
  if rollout and mode in ('coop', 'team'):
    raise ValueError('rollout=True is built for the one-env-per-lane kernel '
                     '(mode auto, unrolled or rolled), not for mode=%r' % mode)
  per_env = codegen.normalise_per_env(per_env)     # ValueError: unknown names
  if per_env and mode == 'team':
    raise codegen.UnsupportedModelError(
        'per_env: per-env model fields are not implemented for mode="team" (big '
        'scenes, soccer); build the team scene without per_env')
  if precision not in ('f32', 'f64', 'mixed'):
    raise ValueError('precision must be "f32", "f64" or "mixed"')
  if mode not in ('auto', 'unrolled', 'rolled', 'coop', 'team'):
    raise ValueError('mode must be auto, unrolled, rolled, coop or team')
  if task == codegen.TASK_SOCCER and mode not in ('team', 'rolled'):
    raise ValueError('TASK_SOCCER is an output stage of the team kernel (mode "team", or '
                     '"rolled": the same source with one lane), not of mode=%r' % mode)
  if task == codegen.TASK_SOCCER and (rollout or precision == 'mixed'):
    raise ValueError('TASK_SOCCER has no rollout and no mixed-precision build')
  if precision == 'mixed' and mode in ('coop', 'team'):
    raise ValueError('precision "mixed" is built for the one-env-per-lane kernel')
  if extra_flags is None:
    # experiment hook: extra -D flags for ablation builds (never set in tests)
    extra_flags = os.environ.get('DMC_EXTRA_FLAGS', '').split()
  flags = tuple(extra_flags)
  if mode == 'team':
    # big scenes: the generic source with one wavefront per env (csrc/dmc_kernels.hip,
    # "team mode"): matrices, rows and contacts in the HBM workspace, a tree's
    # diagonal block at a time in LDS
    flags += ('-DDMC_TEAM=64',)
  if precision == 'mixed':
    # fp32 arithmetic, qpos/qvel carried between steps as fp64 (high, low)
    # pairs (csrc/dmc_kernels.hip, DMC_STATE_COMP); one-env-per-lane kernel only
    flags += ('-DDMC_STATE_COMP=1',)
  if mode == 'coop':
    # several lanes per env (csrc/dmc_coop.hip): working set in LDS, generic
    # loops; `lds_budget` does not apply (no row tiers)
    flags = tuple(f for f in flags if not f.startswith('-DDMC_LDS_BUDGET'))
    if group not in (8, 16, 32, 64, 128):
      raise ValueError('group must be 8, 16, 32, 64 or 128 (two wavefronts) lanes per env')
    # 128: one env per 64 lanes plus a second wavefront that builds the
    # constraint rows and factorises M + h D meanwhile (Euler models; the best
    # shape while the batch fits the chip in one round, 4 envs per CU)
    flags += ('-DDMC_GROUP=%d' % min(group, 64), '-DDMC_COOP_DUO=%d' % (group == 128))
    source, tiers = 'dmc_coop.hip', (_COOP,)
  else:
    if lds_budget is not None and lds_budget != 128*1024:
      flags += ('-DDMC_LDS_BUDGET=%d' % lds_budget,)
    semi = (model.nv <= SEMI_ROLLED_MAX_NV     # (experiments: skip this tier)
            and os.environ.get('DMC_ROLLED_STRICT') != '1')
    tiers = (_SEMI, _ROLLED) if semi else (_ROLLED,)
    if mode in ('auto', 'unrolled'):
      tiers = (_UNROLLED,) + tiers if mode == 'auto' else (_UNROLLED,)
    source = 'dmc_kernels.hip'
  if rollout:
    # per-step outputs and the device MLP policy (csrc/dmc_kernels.hip, DMC_ROLLOUT)
    flags += ('-DDMC_ROLLOUT=1',)
  if population:
    # one policy per group of envs (csrc/dmc_kernels.hip, DMC_POLICY_POPULATION)
    flags += ('-DDMC_POLICY_POPULATION=1',)
  return Spec(model, task, ncon_max, precision, mode, group, lds_budget, source,
              'f64' if precision == 'f64' else 'f32', flags, tiers, per_env)


def _flags(spec_, tier, remarks=False):
  """The compiler flags of one tier of `spec_`: the only place that knows them
  (hipcc, the in-process route and `code_object_bytes` all come here).
  `remarks`: have the resource usage reported, for `_spills`.  The order is
  part of the result: clang hashes its command line into the code object.

  -pragma-unroll-threshold: the per-model straight-line code is far beyond
    LLVM's default budget; without it the pair loop stays rolled, per-lane
    arrays are indexed dynamically and the whole working set lands in scratch.
  -fno-slp-vectorize: v_pk_*_f32 is not faster on gfx950 and the packing
    moves cost ~25 % extra instructions plus spills.
  -fno-hip-fp32-correctly-rounded-divide-sqrt (fp32 build only): v_rcp/v_rsq
    based division and sqrt (<= 2.5 ulp) instead of the 10-instruction
    IEEE sequences; the fp64 build keeps exact division.
  -ffinite-math-only -fno-signed-zeros: lets LLVM fold 0*x and x+0.  In the
    unrolled build the world frame, joint axes and body offsets are
    constants, so for the planar suite models (cheetah, walker, hopper,
    cart-pole, ...) the y components, two quaternion entries and four matrix
    entries of every frame are exact zeros that now disappear at compile time
    (cheetah: 25.4 k -> 18.6 k VALU instructions per step).  Values are
    unchanged for finite inputs; NaN/inf detection is done on bit patterns
    (`bad()` in the kernel source), not with comparisons.
  """
  f64 = spec_.real == 'f64'
  flags = ['-DDMC_REAL_IS_DOUBLE'] if f64 else list(_FP32_FLAGS)
  flags += list(spec_.flags) + [
      '--offload-arch=' + ARCH, '-O3', '-std=c++17',
      '-ffinite-math-only', '-fno-signed-zeros'] + (
          ['-Rpass-analysis=kernel-resource-usage'] if remarks else []) + [
      '-mllvm', '-pragma-unroll-threshold=%s' % os.environ.get(
          'DMC_PRAGMA_UNROLL_THRESHOLD', '10000000'), '-fno-slp-vectorize',
      '-ffp-contract=off' if f64 else '-ffp-contract=fast']
  if tier.unroll is False:   # ("semi": generic source, the backend may unroll)
    flags += list(_ROLLED_FLAGS)
  return flags


def _key(spec_, tier):
  return model_key(spec_.model, spec_.task, spec_.real, spec_.ncon_max,
                   spec_.flags, tier.unroll, spec_.per_env)


def _compile(spec_, tier, out, keep_temps):
  """Compiles one tier of `spec_` to `out + '.tmp'` (header and temporaries next
  to it); returns its (vgpr, sgpr) spill counts, see `_spills`."""
  model = spec_.model
  if os.environ.get('DMC_BUILD_LOG'):     # which code objects were not pre-built
    with open(os.environ['DMC_BUILD_LOG'], 'a') as f:
      f.write('%s task=%d %s ncon_max=%r flags=%r unroll=%r nv=%d nbody=%d\n' % (
          spec_.source, spec_.task, spec_.real, spec_.ncon_max, spec_.flags,
          tier.unroll, model.nv, model.nbody))
  header = os.path.join(os.path.dirname(out), 'model_%s.h' % _key(spec_, tier))
  text = codegen.generate_header(model, spec_.task, spec_.ncon_max,
                                 unroll=tier.unroll is True, per_env=spec_.per_env)
  with open(header, 'w') as f:
    f.write(text)
  flags = _flags(spec_, tier, remarks=True)
  if backend() == 'hiprtc':
    code, log = _compile_in_process(text, spec_.source, flags)
    with open(out + '.tmp', 'wb') as f:
      f.write(code)
  else:
    cmd = [_hipcc(), '--genco'] + flags + [
        '-DDMC_MODEL_HEADER="%s"' % header, '-I', _CSRC,
        '-o', out + '.tmp', os.path.join(_CSRC, spec_.source)]
    if keep_temps:
      cmd.insert(1, '-save-temps')
    proc = subprocess.run(cmd, cwd=os.path.dirname(out), stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, universal_newlines=True)
    if proc.returncode != 0:
      raise RuntimeError('hipcc failed for model kernels:\n%s'
                         % proc.stdout[-4000:])
    log = proc.stdout
  if keep_temps:
    print(log)
  return _spills(log)


def _compile_in_process(header_text, source, flags):
  """No toolchain driver: the C ABI compiles the same source with the same
  flags in-process (`dmc_model_compile`, HIP runtime compilation); the headers
  travel as text."""
  from dm_control_amd import wrapper
  headers = {'model.h': header_text}
  for name in ('dmc_args.h', 'dmc_kernels.hip'):
    if name != source:
      with open(os.path.join(_CSRC, name)) as f:
        headers[name] = f.read()
  with open(os.path.join(_CSRC, source)) as f:
    text = f.read()
  return wrapper.compile_code_object(
      text, source, headers, list(flags) + ['-DDMC_MODEL_HEADER="model.h"'])


def code_object_bytes(model, task=codegen.TASK_NONE, precision='f32',
                      ncon_max=None, unroll=False, coop_group=None, per_env=()):
  """gfx950 code object of `model` as bytes, built in-process (no hipcc, no
  files): the `mj_loadXML` route for a model that was not pre-built --
  `wrapper.HipModel.from_code(build.code_object_bytes(model))`.  The generic
  (rolled) build by default: it compiles in seconds for any model size."""
  mode = 'coop' if coop_group else 'unrolled' if unroll else 'rolled'
  spec_ = spec(model, task, precision, ncon_max, (), mode, None, coop_group or 64,
               per_env)
  tier = spec_.tiers[-1]        # no spill counts on this route: strictly rolled
  header = codegen.generate_header(model, task, ncon_max, unroll=tier.unroll is True,
                                   per_env=spec_.per_env)
  return _compile_in_process(header, spec_.source, _flags(spec_, tier))[0]


def lds_budget_for(nenv):
  """LDS bytes per workgroup for the constraint-row / contact staging area.

  The step kernel is bound by VALU issue of one wave per SIMD, so how many
  workgroups fit on a CU decides the throughput once the batch exceeds one
  wave per CU.  Measured on cheetah-run (M env-steps/s at 128 / 64 / 36-40 KB):
  B = 8192: 102 / 101 / 85;  16384: 201 / 198 / 169;  32768: 217 / 374 / 319;
  65536: 228 / 404 / 583;  262144: 248 / 456 / 657.
  """
  if nenv is None or nenv <= 16384:
    return 128*1024         # 1 workgroup per CU, most rows in LDS
  if nenv <= 32768:
    return 64*1024          # 2 per CU
  return 36*1024            # 4 per CU: one wave on every SIMD


def _recorded(out):
  """The verdict on record for the code object `out`, from its sidecar file:
  ("ok" | "over" | "nolds", spill counts as text), or (None, None)."""
  try:
    with open(out + '.verdict') as f:
      verdict, _, counts = f.read().strip().partition(' ')
  except FileNotFoundError:
    return None, None
  return (verdict, counts) if verdict in ('ok', 'over', 'nolds') else (None, None)


def _accepted(verdict, last):
  """Within budget; beyond it only as the last tier of a request made under
  `allow_overbudget()` -- never as a step of "auto"."""
  return verdict == 'ok' or (verdict == 'over' and last and _allow_overbudget())


def realise(spec_, force=False, keep_temps=False):
  """Walks the tiers of `spec_` (module docstring, "The ladder") and returns the
  path of the first code object whose verdict is accepted.  `force`: ignore the
  verdicts on record, i.e. compile every tier visited again."""
  os.makedirs(_BUILD, exist_ok=True)
  for tier in spec_.tiers:
    last = tier is spec_.tiers[-1]
    out = os.path.join(_BUILD, 'dmc_%s.hsaco' % _key(spec_, tier))
    verdict, counts = (None, None) if force else _recorded(out)
    if verdict is None or (_accepted(verdict, last) and not os.path.exists(out)):
      try:
        spills = _compile(spec_, tier, out, keep_temps)
      except RuntimeError as e:
        if 'does not fit in LDS' not in str(e):
          raise
        # static_assert of csrc/dmc_coop.hip: ENV_WORDS*EPB*sizeof(real) > 150 KB
        verdict, counts = 'nolds', ''
      else:
        verdict = 'ok' if _within_spill_budget(spills, tier.max_sgpr) else 'over'
        counts = '%r' % (spills,)
      with open(out + '.verdict', 'w') as f:
        f.write('%s %s\n' % (verdict, counts))
      if _accepted(verdict, last):
        os.replace(out + '.tmp', out)
      elif verdict != 'nolds':
        os.remove(out + '.tmp')
    if verdict == 'nolds':
      raise LdsWorkingSetError(_LDS_MSG % (
          spec_.group, spec_.real, 64//min(spec_.group, 64)))
    if _accepted(verdict, last):
      return out
    if last:
      raise RuntimeError(tier.refusal % counts)


def build_model(model, task=codegen.TASK_NONE, precision='f32',
                ncon_max=None, force=False, keep_temps=False, extra_flags=None,
                mode='auto', lds_budget=None, group=64, per_env=(), rollout=False,
                population=False):
  """Generates the constants header for `model` and compiles its kernels.

  mode: "unrolled" (static indexing, per-lane state in registers), "rolled"
  (generic loops, per-lane arrays in scratch) or "auto" (unrolled unless its
  register spills exceed MAX_*_SPILLS), "team" (the rolled source with the 64
  lanes of a wavefront sharing ONE env: scenes whose matrices live in the HBM
  workspace, e.g. a soccer pitch), or "coop": `group` lanes advance one
  env together with its working set in LDS (csrc/dmc_coop.hip; the shape for
  nv ~ 20+ models and for small shards; 128 = 64 lanes + a helper wavefront).  Returns the path of the gfx950 code
  object; cached in-tree by content hash.

  per_env: names of model fields (codegen.PER_ENV_FIELDS) that the kernels read
  per env from the model-parameter block (DMC_FIELD_MODELPARAM) instead of the
  compiled tables; () builds what a build without the argument builds.  A
  varied build walks the same tiers: where its extra loads push it past the
  spill budget of a tier the default build fits, its `.verdict` says "over" and
  the next tier is taken.

  rollout: True builds the rollout variant of the one-env-per-lane kernel
  (`dmc_batch_rollout`: per-step outputs, device MLP policy); it walks the same
  tiers and is refused (ValueError) for "coop" and "team".

  population: True (with rollout=True, else a ValueError) builds the rollout
  variant that takes a population of policies (`dmc_batch_rollout_population`:
  env e acts with the weights of member e // (nenv // P)); the same tiers.
  """
  return realise(spec(model, task, precision, ncon_max, extra_flags, mode,
                      lds_budget, group, per_env, rollout, population), force, keep_temps)
