"""The code objects the product can select, as an explicit list.

`engine.Physics` picks one gfx950 code object from (domain, precision, batch
size): the one-env-per-lane kernel (csrc/dmc_kernels.hip, mode "auto") in one
of three LDS budgets (`build.lds_budget_for`), or the several-lanes-per-env
kernel (csrc/dmc_coop.hip, mode "coop") with 128, 64 or 32 lanes per env
(`_COOP_POLICY`, `_COOP_POLICY_F64` of the domain's Physics subclass).

`SHIPPED` is that choice written down, one selection per line.
`enumerate_selections()` derives the same list from the product;
tests/test_selection.py asserts the two are equal, and
tests/test_gpu_selection.py runs every line on the device (per-step parity
with the oracle, and the selection itself at the batch sizes that select it).
A policy edit therefore fails on the CPU until the new shape has its line
here, and the line brings its device runs with it.

Not in the matrix: `locomotion.soccer` (build mode "team", f32 / f64) is
selected by class, not by batch size.  Its code objects are compared with the
oracle by tests/test_soccer_model.py
(test_pitch_build_per_step_parity_with_oracle, test_team_build_*,
test_soccer_load_other_team_sizes_match_oracle) and
tests/test_soccer_task.py.
"""

from unittest import mock

from dm_control_amd import build
from dm_control_amd import engine
from dm_control_amd import suite

KB = 1024
PRECISIONS = ('f32', 'f64', 'mixed')
REFUSED = 'refused'     # mode of a line whose build_model call raises ValueError
OPEN_ENDED_BATCH = 262144   # the largest batch the enumeration visits

# (domain, precision, mode, group or None, lds_budget or None, lo_batch,
#  hi_batch): lo / hi are the smallest and largest batch size that select the
# line; hi_batch None = the open-ended last tier.  Mode "coop" takes no LDS
# budget (the several-lanes kernel has no row tiers), mode "auto" no group.
SHIPPED = (
    ('acrobot', 'f32', 'auto', None, 128*KB, 1, 16384),
    ('acrobot', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('acrobot', 'f32', 'auto', None, 36*KB, 32769, None),
    ('acrobot', 'f64', 'auto', None, 128*KB, 1, 16384),
    ('acrobot', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('acrobot', 'f64', 'auto', None, 36*KB, 32769, None),
    ('acrobot', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('acrobot', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('acrobot', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('cartpole', 'f32', 'auto', None, 128*KB, 1, 16384),
    ('cartpole', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('cartpole', 'f32', 'auto', None, 36*KB, 32769, None),
    ('cartpole', 'f64', 'auto', None, 128*KB, 1, 16384),
    ('cartpole', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('cartpole', 'f64', 'auto', None, 36*KB, 32769, None),
    ('cartpole', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('cartpole', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('cartpole', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('cheetah', 'f32', 'coop', 128, None, 1, 1024),
    ('cheetah', 'f32', 'coop', 64, None, 1025, 2048),
    ('cheetah', 'f32', 'auto', None, 128*KB, 2049, 16384),
    ('cheetah', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('cheetah', 'f32', 'auto', None, 36*KB, 32769, None),
    ('cheetah', 'f64', 'coop', 128, None, 1, 4096),
    ('cheetah', 'f64', 'auto', None, 128*KB, 4097, 16384),
    ('cheetah', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('cheetah', 'f64', 'auto', None, 36*KB, 32769, None),
    ('cheetah', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('cheetah', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('cheetah', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('hopper', 'f32', 'coop', 128, None, 1, 1024),
    ('hopper', 'f32', 'coop', 64, None, 1025, 2048),
    ('hopper', 'f32', 'coop', 32, None, 2049, 4096),
    ('hopper', 'f32', 'auto', None, 128*KB, 4097, 16384),
    ('hopper', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('hopper', 'f32', 'auto', None, 36*KB, 32769, None),
    ('hopper', 'f64', 'coop', 128, None, 1, 1024),
    ('hopper', 'f64', 'coop', 32, None, 1025, 8192),
    ('hopper', 'f64', 'auto', None, 128*KB, 8193, 16384),
    ('hopper', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('hopper', 'f64', 'auto', None, 36*KB, 32769, None),
    ('hopper', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('hopper', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('hopper', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('humanoid', 'f32', 'coop', 128, None, 1, None),
    ('humanoid', 'f64', 'coop', 128, None, 1, None),
    ('humanoid', 'mixed', REFUSED, None, None, 1, None),
    ('pendulum', 'f32', 'auto', None, 128*KB, 1, 16384),
    ('pendulum', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('pendulum', 'f32', 'auto', None, 36*KB, 32769, None),
    ('pendulum', 'f64', 'auto', None, 128*KB, 1, 16384),
    ('pendulum', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('pendulum', 'f64', 'auto', None, 36*KB, 32769, None),
    ('pendulum', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('pendulum', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('pendulum', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('point_mass', 'f32', 'auto', None, 128*KB, 1, 16384),
    ('point_mass', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('point_mass', 'f32', 'auto', None, 36*KB, 32769, None),
    ('point_mass', 'f64', 'auto', None, 128*KB, 1, 16384),
    ('point_mass', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('point_mass', 'f64', 'auto', None, 36*KB, 32769, None),
    ('point_mass', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('point_mass', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('point_mass', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('reacher', 'f32', 'auto', None, 128*KB, 1, 16384),
    ('reacher', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('reacher', 'f32', 'auto', None, 36*KB, 32769, None),
    ('reacher', 'f64', 'auto', None, 128*KB, 1, 16384),
    ('reacher', 'f64', 'auto', None, 64*KB, 16385, 32768),
    ('reacher', 'f64', 'auto', None, 36*KB, 32769, None),
    ('reacher', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('reacher', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('reacher', 'mixed', 'auto', None, 36*KB, 32769, None),
    ('walker', 'f32', 'coop', 128, None, 1, 1024),
    ('walker', 'f32', 'coop', 64, None, 1025, 2048),
    ('walker', 'f32', 'coop', 32, None, 2049, 8192),
    ('walker', 'f32', 'auto', None, 128*KB, 8193, 16384),
    ('walker', 'f32', 'auto', None, 64*KB, 16385, 32768),
    ('walker', 'f32', 'auto', None, 36*KB, 32769, None),
    ('walker', 'f64', 'coop', 128, None, 1, 1024),
    ('walker', 'f64', 'coop', 32, None, 1025, 32768),
    ('walker', 'f64', 'auto', None, 36*KB, 32769, None),
    ('walker', 'mixed', 'auto', None, 128*KB, 1, 16384),
    ('walker', 'mixed', 'auto', None, 64*KB, 16385, 32768),
    ('walker', 'mixed', 'auto', None, 36*KB, 32769, None),
)

# 8 and 16 lanes per env are not a policy choice but a public keyword
# (`environment_kwargs={'build_mode': 'coop', 'group': 8}`): the models with
# few enough dofs to make them plausible, (domain, group, precision).
SMALL_GROUPS = tuple((domain, group, precision)
                     for domain in ('cheetah', 'hopper', 'walker')
                     for group in (8, 16) for precision in ('f32', 'f64'))
# ... of which `build_model` refuses these (`build.LdsWorkingSetError`, a
# ValueError): the working sets of 64/group envs do not fit one workgroup's LDS
SMALL_GROUPS_REFUSED = (('cheetah', 8, 'f64'),)


class _Recorded(Exception):
  """Raised in place of the compile; `args[0]` is the spec that was asked for."""


def _refuse_to_compile(spec, force=False, keep_temps=False):
  raise _Recorded(spec)


def recording():
  """Inside, `build.realise` raises `_Recorded` with the spec it receives
  instead of compiling; `build.spec` has checked the arguments by then."""
  return mock.patch.object(build, 'realise', _refuse_to_compile)


def _subclasses(cls):
  for sub in cls.__subclasses__():
    yield sub
    yield from _subclasses(sub)


def policy_boundaries():
  """Every batch size at which some Physics subclass changes shape, read from
  the classes, plus the LDS budget boundaries."""
  bounds = {16384, 32768}
  for cls in _subclasses(engine.Physics):
    for policy in (cls._COOP_POLICY, cls._COOP_POLICY_F64):   # pylint: disable=protected-access
      bounds.update(max_batch for max_batch, _ in policy or ())
  return sorted(bounds)


def first_task(domain):
  return next(task for d, task in suite.ALL_TASKS if d == domain)


def select(domain, precision, batch_size):
  """(mode, group or None, lds_budget or None) of what `suite.load` builds for
  this batch size; mode REFUSED if `build_model` raises ValueError."""
  with recording():
    try:
      suite.load(domain, first_task(domain), environment_kwargs={
          'batch_size': batch_size, 'precision': precision})
    except _Recorded as recorded:
      spec = recorded.args[0]
    except ValueError:
      return REFUSED, None, None
    else:
      raise AssertionError('suite.load(%r) built nothing' % domain)
  assert spec.precision == precision
  if spec.mode == 'coop':
    return spec.mode, spec.group, None
  return spec.mode, None, spec.lds_budget


def enumerate_selections():
  """The list `SHIPPED` should be, derived from the product."""
  bounds = policy_boundaries()
  sizes = sorted({1, OPEN_ENDED_BATCH} | set(bounds) | {b + 1 for b in bounds})
  out = []
  for domain in sorted({d for d, _ in suite.ALL_TASKS}):
    for precision in PRECISIONS:
      runs = []      # [selection, lo, hi] in increasing batch size
      for b in sizes:
        sel = select(domain, precision, b)
        if runs and runs[-1][0] == sel:
          runs[-1][2] = b
        else:
          runs.append([sel, b, b])
      for sel, lo, hi in runs:
        out.append((domain, precision) + sel + (lo, None if hi == sizes[-1] else hi))
  return tuple(out)


def build_args(line):
  """Keyword arguments of `build.build_model` for a line of SHIPPED."""
  _, precision, mode, group, lds_budget, _, _ = line
  kwargs = {'precision': precision, 'mode': mode}
  if group is not None:
    kwargs['group'] = group
  if lds_budget is not None:
    kwargs['lds_budget'] = lds_budget
  return kwargs


def line_id(line):
  domain, precision, mode, group, lds_budget, _, _ = line
  shape = 'g%d' % group if group else (
      'lds%dk' % (lds_budget//KB) if lds_budget else mode)
  return '%s-%s-%s' % (domain, precision, shape)


if __name__ == '__main__':
  for row in enumerate_selections():
    print('    %r,' % (row,))
