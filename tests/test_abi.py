"""The C-ABI library loads and exports every symbol include/dmc_hip.h declares, and
the copies of its contract (fields, model info, flag bits) agree with it."""

import ctypes
import os
import re

import pytest

from dm_control_amd import build
from dm_control_amd import wrapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
  with open(os.path.join(ROOT, 'include', 'dmc_hip.h')) as f:
    text = f.read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return sorted(set(re.findall(r'\b(dmc_[a-z_0-9]+)\s*\(', text)))


def test_header_symbols_are_exported_and_bound():
  build.build_library()
  lib = ctypes.CDLL(wrapper.get_lib_path())
  names = _declared_functions()
  assert len(names) >= 20
  for name in names:
    assert hasattr(lib, name), 'libdmc_hip.so does not export %s' % name
  # the ctypes shim binds exactly the declared surface
  assert sorted(wrapper.SIGNATURES) == names


def test_version_and_error_channel_without_device():
  lib = wrapper.get_lib()
  assert lib.dmc_version() >= 100
  assert lib.dmc_device_count() >= 0
  if lib.dmc_device_count() == 0:
    ptr = ctypes.c_void_p()
    rc = lib.dmc_model_load(b'/nonexistent.hsaco', 0, ctypes.byref(ptr))
    assert rc != 0
    assert b'no HIP device' in lib.dmc_last_error()


def test_in_process_compile_needs_no_toolchain_and_reports_errors():
  """dmc_model_compile (the compile half of mj_loadXML at the C boundary): HIP
  runtime compilation inside libdmc_hip.so -- no hipcc executable, no files, no
  GPU.  A model that was never pre-built becomes a gfx950 code object (an ELF
  image); a broken source fails with the compiler's log, like the
  `char error[1000]` of mj_loadXML (wrapper/core.py:312-328)."""
  import kat_models
  from dm_control_amd import build
  from dm_control_amd.mjcf import compiler
  model = compiler.from_xml_string(kat_models.GPU_MODELS['ball_on_floor'])
  code = build.code_object_bytes(model, 0, 'f64')
  assert code[:4] == b'\x7fELF' and len(code) > 10000
  with pytest.raises(wrapper.Error) as err:
    wrapper.compile_code_object('__global__ void k() { this is not C++; }', 'bad.hip',
                                {}, ['--offload-arch=gfx950'])
  assert 'error' in str(err.value)


# -- one definition each: the header, the device contract and the Python mirror --

CSRC = os.path.join(ROOT, 'dm_control_amd', 'csrc')


def _text(*path):
  with open(os.path.join(*path)) as f:
    return f.read()


def _header():
  return re.sub(r'/\*.*?\*/', '', _text(ROOT, 'include', 'dmc_hip.h'), flags=re.S)


def _defines(text, prefix):
  return {n: int(v) for n, v in re.findall(r'#define\s+(%s\w+)\s+(\d+)\b' % prefix, text)}


def test_python_field_table_is_the_header_enum():
  body = re.search(r'enum\s+dmc_field\s*\{(.*?)\}', _header(), flags=re.S).group(1)
  enum = [(n, int(v)) for n, v in re.findall(r'DMC_FIELD_(\w+)\s*=\s*(\d+)', body)]
  assert enum[-1] == ('COUNT', len(wrapper.FIELDS)) and len(enum) == 17
  assert enum[:-1] == [(f[0], k) for k, f in enumerate(wrapper.FIELDS)]
  for name, value in enum[:-1]:
    assert getattr(wrapper, 'FIELD_' + name) == value


def test_python_model_info_is_the_header_struct():
  body = re.search(r'typedef\s+struct\s+dmc_model_info\s*\{(.*?)\}', _header(),
                   flags=re.S).group(1)
  decl = re.fullmatch(r'\s*int\b([^;]*);\s*', body)     # one declaration, all int
  members = [m.strip() for m in decl.group(1).split(',')]
  assert len(members) == 20
  assert members == [n for n, _ in wrapper.ModelInfo._fields_]
  assert all(t is ctypes.c_int for _, t in wrapper.ModelInfo._fields_)


def test_named_constants_agree():
  step = _defines(_header(), 'DMC_STEP_')
  assert step == {'DMC_STEP_OUTPUTS': wrapper.STEP_OUTPUTS,
                  'DMC_STEP_STALE_FIRST': wrapper.STEP_STALE_FIRST}
  flags = _defines(_text(CSRC, 'dmc_args.h'), 'DMC_FLAG_')
  assert len(flags) >= 7
  assert all(v > 0 and v & (v - 1) == 0 for v in flags.values()), flags
  assert len(set(flags.values())) == len(flags), flags


def test_sources_name_the_contract():
  """Our own idiom, searched as text: no kernel tests a bare flag bit and the
  host decodes no dmc_info entry by position."""
  for name in ('dmc_kernels.hip', 'dmc_coop.hip'):
    assert not re.findall(r'flags\s*&\s*\d.*', _text(CSRC, name)), name
  assert 'raw[' not in _text(CSRC, 'dmc_api.cpp')


def _contract_builds():
  import helpers
  import model_param_cases as mpc
  return {
      'one_lane': ('cartpole', dict(precision='f32')),
      'several_lanes': ('hopper', dict(precision='f32', mode='coop', group=32)),
      'per_env': ('cheetah', dict(precision='f32', mode='coop', group=64,
                                  per_env=mpc.ALL_FIELDS)),
  }, helpers


WRITABLE = ('QPOS', 'QVEL', 'WARMSTART', 'TIME', 'CTRL', 'TASKDATA', 'MODELPARAM',
            'RETURN', 'WARN')


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['one_lane', 'several_lanes', 'per_env'])
def test_field_table_on_the_device(which):
  """3 envs (a ragged fraction of a workgroup; two envs per workgroup, env-major;
  a model-parameter block of several rows): every field has the size of the
  Python table, the refused ones are refused and leave a batch that steps, the
  writable ones come back bit for bit as the [k][nenv] array written."""
  import numpy as np
  builds, helpers = _contract_builds()
  domain, kw = builds[which]
  hm = wrapper.HipModel(build.build_model(helpers.load_model(domain),
                                          helpers.TASKS[domain], **kw))
  hb = wrapper.HipBatch(hm, 3)
  info = hm.info
  assert (info.lanes_per_env > 1, bool(info.env_major), info.nmodelparam > 1) == {
      'one_lane': (False, False, False), 'several_lanes': (True, True, False),
      'per_env': (True, True, True)}[which]
  lib = wrapper.get_lib()
  for f in range(len(wrapper.FIELDS)):
    shape, dtype = hb._shape(f), np.dtype(hb._dtype(f))   # pylint: disable=protected-access
    assert lib.dmc_batch_field_bytes(hb.ptr, f) == int(np.prod(shape))*dtype.itemsize
  assert lib.dmc_batch_field_bytes(hb.ptr, len(wrapper.FIELDS)) == 0
  word = np.zeros(1, np.float32)
  for f, row in enumerate(wrapper.FIELDS):
    if row[0] not in WRITABLE:
      with pytest.raises(wrapper.Error, match='field %d is not writable' % f):
        hb.write(f, np.zeros(hb._shape(f)))               # pylint: disable=protected-access
  for f in (-1, len(wrapper.FIELDS)):
    assert lib.dmc_batch_write(hb.ptr, f, word.ctypes.data, word.nbytes) != 0
    assert b'field %d is not writable' % f in lib.dmc_last_error()
  t0 = hb.read(wrapper.FIELD_TIME)
  hb.step_host(np.zeros((3, info.nu)), 1)
  assert np.all(hb.read(wrapper.FIELD_TIME) > t0)
  assert np.all(np.isfinite(hb.read(wrapper.FIELD_QPOS)))
  for f, row in enumerate(wrapper.FIELDS):
    if row[0] in WRITABLE:
      shape, dtype = hb._shape(f), hb._dtype(f)           # pylint: disable=protected-access
      # distinct and exact in fp32: 100 f + 1, 100 f + 1.25, ...
      sent = (100*f + 1 + 0.25*np.arange(np.prod(shape))).reshape(shape)
      if row[4] != 'real':
        sent = 100*f + 1 + np.arange(np.prod(shape)).reshape(shape)
      sent = sent.astype(dtype)
      assert len(np.unique(sent)) == sent.size
      hb.write(f, sent)
      got = hb.read(f)
      assert got.dtype == sent.dtype and got.tobytes() == sent.tobytes(), row[0]
  hb.free()
  hm.free()
