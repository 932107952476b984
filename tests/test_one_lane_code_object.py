"""What the compiler made of the shipped one-env-per-lane fp32 step kernels
(cheetah, hopper; the default build of `Physics`): cross-compiled here, no GPU.

  * `dmc_step` and `dmc_observe` keep nothing in scratch memory
    (`private_segment_fixed_size` 0 in the code object's metadata): the frame of a
    contact candidate stays in registers (csrc/dmc_kernels.hip, sphere_sphere);
  * the build is still the first tier of the ladder (unrolled, within the spill
    budget), not a fall-back to the generic source;
  * `dmc_step` takes no more registers (VGPRs, AGPRs included) and spills no more
    SGPRs than the figures on record in profiles/one_lane_fp32_code_object.json,
    measured on the commit before the candidates left scratch.
"""

import json
import os
import re
import shutil
import subprocess

import pytest

import helpers
from dm_control_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'profiles', 'one_lane_fp32_code_object.json')) as _f:
  RECORD = json.load(_f)


def _readelf():
  exe = shutil.which('llvm-readelf')
  if exe:
    return exe
  rocm = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))   # pylint: disable=protected-access
  for sub in ('llvm/bin', 'lib/llvm/bin'):
    exe = os.path.join(rocm, sub, 'llvm-readelf')
    if os.path.exists(exe):
      return exe
  raise RuntimeError('llvm-readelf not found next to hipcc')


def kernel_metadata(code_object, tmp_path):
  """{kernel name: {metadata key: int}} of a code object (an offload bundle
  around one gfx950 ELF), from the AMDGPU metadata note."""
  with open(code_object, 'rb') as f:
    data = f.read()
  elf = tmp_path/'code_object.elf'
  elf.write_bytes(data[data.index(b'\x7fELF'):])
  notes = subprocess.run([_readelf(), '--notes', str(elf)], stdout=subprocess.PIPE,
                         universal_newlines=True, check=True).stdout
  kernels = {}
  for block in re.split(r'\n  - (?=\.agpr_count:)', notes)[1:]:
    name = re.search(r'\.name:\s+(\w+)', block).group(1)
    kernels[name] = {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s*$', block, re.M)}
  return kernels


@pytest.mark.parametrize('domain', ['cheetah', 'hopper'])
def test_default_fp32_build_keeps_its_tier_and_uses_no_scratch(domain, tmp_path):
  model, task = helpers.load_model(domain), helpers.TASKS[domain]
  spec = build.spec(model, task, 'f32', None, (), 'auto', None, 64)
  path = build.realise(spec)
  # the first tier: the unrolled source, within the spill budget
  assert os.path.basename(path) == 'dmc_%s.hsaco' % build._key(spec, spec.tiers[0])   # pylint: disable=protected-access
  assert spec.tiers[0].unroll is True
  with open(path + '.verdict') as f:
    assert f.read().split()[0] == 'ok'
  meta = kernel_metadata(path, tmp_path)
  for kernel in ('dmc_step', 'dmc_observe'):
    assert meta[kernel]['private_segment_fixed_size'] == 0, (kernel, meta[kernel])
    assert meta[kernel]['vgpr_spill_count'] == 0, (kernel, meta[kernel])
  before = RECORD[domain]['before']['dmc_step']
  step = meta['dmc_step']
  print(domain, step)
  assert before['private_segment_fixed_size'] > 0       # (what the record is about)
  assert step['vgpr_count'] <= before['vgpr_count']
  assert step['sgpr_spill_count'] <= before['sgpr_spill_count']
