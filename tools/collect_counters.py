"""Assembles profiles/counters_<code object>_b<batch>.json from the rocprofv3
`--pmc` passes of one bench workload (tools/r02_measure.sh), keyed by the code
object the passes ran on -- bench.py only reports counter figures whose code
object matches the one it is running (profiles/README.md).

  python tools/collect_counters.py <gpurun_out/measure dir> <tag> <bench json line file>
      [control steps per launch]

A launch of the one-env-per-lane kernel covers a chunk of control steps (bench.py
issues chunks of 16; DESIGN.md 5, sequence launches), while bench.py sets the
figures of this file against its time per control step.  So `counters` keeps the
medians per dmc_step launch as measured, and everything derived from them
(`traffic_bytes_per_launch`, `valu_insts_per_launch`: the names bench.py reads)
is per control step: divided by the steps of the median launch, 16 for that
kernel shape unless the fourth argument says otherwise, 1 for the shapes that
take one launch per step.

Unit corrections (MI355X_MICROARCH.md, HBM / rocprofv3): FETCH_SIZE and
WRITE_SIZE are in KB per launch as rocprofv3 reports them; on gfx950 FETCH_SIZE
counts wide (16-byte per lane) coalesced streaming reads at half their bytes --
the step kernel's loads are 4-byte per lane, coalesced over the wave, for which
the counter is exact, so no correction is applied (stated in the output).
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pmc(directory):
  out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rocprof_summary.py'),
                        'pmc', directory], stdout=subprocess.PIPE, universal_newlines=True)
  try:
    return json.loads(out.stdout.strip().splitlines()[-1])
  except (ValueError, IndexError):
    return {}


SEQ_CHUNK = 16      # bench.py: control steps per call of dmc_batch_step_n


def steps_per_launch(line):
  """Control steps the median dmc_step launch of this bench run covered."""
  one_lane = line['config'].get('kernel_shape', '').startswith('one env per lane')
  return min(SEQ_CHUNK, line['steps']) if one_lane else 1


def main():
  base, tag, bench_file = sys.argv[1:4]
  with open(bench_file) as f:
    line = json.loads([l for l in f if l.startswith('{')][-1])
  code_object = line['config']['code_object']
  batch = line['config']['global_batch']//line['n_gpus']
  counters = {}
  for name in ('FETCH_SIZE', 'WRITE_SIZE', 'SQ_INSTS_VALU', 'SQ_ACTIVE_INST_VALU'):
    counters.update(pmc(os.path.join(base, 'pmc_%s_%s' % (name, tag))))
  med = {k: v['median'] for k, v in counters.items()}
  steps = int(sys.argv[4]) if len(sys.argv) > 4 else steps_per_launch(line)
  out = {
      'code_object': code_object, 'batch': batch, 'workload': line['config']['workload'],
      'control_steps_per_launch': steps,
      'source': 'rocprofv3 --pmc, separate passes, medians per dmc_step launch '
                '(tools/r02_measure.sh)',
      'counters': med}
  if 'FETCH_SIZE' in med and 'WRITE_SIZE' in med:
    out['traffic_bytes_per_launch'] = (med['FETCH_SIZE'] + med['WRITE_SIZE'])*1024/steps
    out['traffic_note'] = ('FETCH_SIZE + WRITE_SIZE (KB) x 1024 / control steps per launch; '
                           '4-byte-per-lane coalesced accesses: no gfx950 wide-read correction applies')
  if 'SQ_INSTS_VALU' in med:
    out['valu_insts_per_launch'] = med['SQ_INSTS_VALU']/steps
  if 'SQ_WAVES' in med:
    out['waves_per_launch'] = med['SQ_WAVES']
  if 'SQ_ACTIVE_INST_VALU' in med and 'SQ_WAVE_CYCLES' in med and med['SQ_WAVE_CYCLES']:
    out['valu_busy'] = med['SQ_ACTIVE_INST_VALU']/med['SQ_WAVE_CYCLES']
  tagname = code_object.replace('dmc_', '').replace('.hsaco', '')
  path = os.path.join(base, 'counters_%s_b%d.json' % (tagname, batch))     # next to the passes
  with open(path, 'w') as f:
    json.dump(out, f, indent=1)
  print(path, json.dumps(out))


if __name__ == '__main__':
  main()
