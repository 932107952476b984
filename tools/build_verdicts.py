"""Tier and spill counts of every suite one-env-per-lane build (no GPU needed).

  python tools/build_verdicts.py [--out FILE] [--extra]

Cross-compiles each suite model in fp32 and fp64 through
`build.build_model(mode='auto')` and prints, per build, the tier of the ladder
that was selected and the (VGPR, SGPR) spill counts on record for every tier
visited.  Two source trees are compared by running this in each and diffing the
output (the code-object keys differ, the lines printed here do not carry them).
`--extra` also builds what the sequence-launch measurements need besides: the
cheetah `mixed` build and the several-lanes builds the policy selects for the
cheetah and the humanoid.
"""

import argparse
import os
import sys
from concurrent import futures

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _ROOT)

import __graft_entry__ as entry  # noqa: E402  pylint: disable=wrong-import-position
from dm_control_amd import build  # noqa: E402  pylint: disable=wrong-import-position

NAMES = ('cartpole', 'cheetah', 'humanoid', 'walker', 'pendulum', 'cartpole-2',
         'cartpole-3', 'acrobot', 'reacher', 'point_mass', 'hopper')
_TIER = {True: 'unrolled', 'semi': 'semi', False: 'rolled'}


def one(name, model, task, precision):
  spec = build.spec(model, task, precision, None, None, 'auto', None, 64)
  path = build.realise(spec)
  visited = []
  chosen = None
  for tier in spec.tiers:
    out = os.path.join(os.path.dirname(path),
                       'dmc_%s.hsaco' % build._key(spec, tier))  # pylint: disable=protected-access
    verdict, counts = build._recorded(out)  # pylint: disable=protected-access
    visited.append('%s=%s%s' % (_TIER[tier.unroll], verdict, counts))
    if out == path:
      chosen = _TIER[tier.unroll]
      break
  return '%-11s %-4s tier=%-8s %s' % (name, precision, chosen, ' '.join(visited))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=None)
  ap.add_argument('--extra', action='store_true')
  ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
  args = ap.parse_args()
  build.build_library()
  models = entry._models()  # pylint: disable=protected-access
  jobs = []
  for name, (model, task, _) in zip(NAMES, models):
    if task == 3:
      continue      # the humanoid has no one-env-per-lane product build
    for precision in ('f32', 'f64'):
      jobs.append((name, model, task, precision))
  lines = []
  with futures.ThreadPoolExecutor(args.jobs) as pool:
    pending = [pool.submit(one, *j) for j in jobs]
    extra = []
    if args.extra:
      extra.append(pool.submit(build.build_model, models[1][0], 2, 'mixed'))
      for model, task, physics in (models[1], models[2]):
        for group in sorted(entry._policy_groups(physics, 'f32')):  # pylint: disable=protected-access
          extra.append(pool.submit(build.build_model, model, task, 'f32',
                                   mode='coop', group=group))
    for f in pending:
      lines.append(f.result())
      print(lines[-1], flush=True)
    for f in extra:
      f.result()
  if args.out:
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
