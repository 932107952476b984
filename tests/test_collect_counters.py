"""tools/collect_counters.py: a dmc_step launch of the one-env-per-lane kernel
covers a chunk of control steps, and what bench.py reads from a counters file
is set against its time per control step."""

import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
  spec = importlib.util.spec_from_file_location(
      'collect_counters', os.path.join(ROOT, 'tools', 'collect_counters.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _line(shape, steps):
  return {'steps': steps, 'n_gpus': 1,
          'config': {'kernel_shape': shape, 'code_object': 'dmc_0123.hsaco', 'global_batch': 8192,
                     'workload': 'cheetah-run'}}


def test_steps_of_the_median_launch():
  tool = _tool()
  one_lane = 'one env per lane (csrc/dmc_kernels.hip)'
  assert tool.steps_per_launch(_line(one_lane, 1000)) == 16
  assert tool.steps_per_launch(_line(one_lane, 5)) == 5        # a run shorter than a chunk
  # one launch per control step: the several-lanes and the team kernels
  assert tool.steps_per_launch(_line('64 lanes per env + a second wavefront (csrc/dmc_coop.hip)', 1000)) == 1
  assert tool.steps_per_launch(_line('one wavefront per env, matrices in the HBM workspace, a tree\'s block '
                                     'at a time in LDS (csrc/dmc_kernels.hip, team mode)', 1000)) == 1


def test_figures_for_bench_are_per_control_step(tmp_path, monkeypatch):
  tool = _tool()
  medians = {'FETCH_SIZE': 3200.0, 'WRITE_SIZE': 1600.0, 'SQ_INSTS_VALU': 20548848.0,
             'SQ_WAVES': 128.0, 'SQ_ACTIVE_INST_VALU': 20837681.0, 'SQ_WAVE_CYCLES': 44039486.0}
  monkeypatch.setattr(tool, 'pmc', lambda directory: {
      k: {'median': v} for k, v in medians.items() if k in os.path.basename(directory) or
      (k in ('SQ_WAVES',) and 'SQ_INSTS_VALU' in directory) or
      (k == 'SQ_WAVE_CYCLES' and 'SQ_ACTIVE_INST_VALU' in directory)})
  bench = tmp_path/'bench.json'
  bench.write_text(json.dumps(_line('one env per lane (csrc/dmc_kernels.hip)', 1000)) + '\n')
  monkeypatch.setattr(sys, 'argv', ['collect_counters.py', str(tmp_path), 'tag', str(bench)])
  tool.main()
  with open(tmp_path/'counters_0123_b8192.json') as f:
    out = json.load(f)
  assert out['control_steps_per_launch'] == 16
  assert out['counters']['SQ_INSTS_VALU'] == medians['SQ_INSTS_VALU']     # as measured, per launch
  assert out['valu_insts_per_launch'] == medians['SQ_INSTS_VALU']/16
  assert out['traffic_bytes_per_launch'] == (3200.0 + 1600.0)*1024/16
  assert out['waves_per_launch'] == 128
  assert abs(out['valu_busy'] - medians['SQ_ACTIVE_INST_VALU']/medians['SQ_WAVE_CYCLES']) < 1e-12
