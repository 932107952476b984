"""The pure half of the host runtime (csrc/dmc_launch.h) without a device: the flags
and members of every kind of launch, the shadow target of an episode prefetch, the
chunks of a sequence and the grid.  tests/host_runtime/launch_plan.cpp is built with
the address and undefined-behaviour sanitizers and run as a program of its own, one
case per run; the device side of the same contract is tests/test_gpu_episode_prefetch.py,
test_gpu_rollout.py and test_gpu_step_sequence.py."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dm_control_amd', 'csrc')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
  exe = str(tmp_path_factory.mktemp('launch_plan')/'launch_plan')
  subprocess.check_call(
      ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
       '-fno-sanitize-recover=undefined', '-Wall', '-I', CSRC,
       os.path.join(ROOT, 'tests', 'host_runtime', 'launch_plan.cpp'), '-o', exe])
  return exe


@pytest.mark.parametrize('case', ['flags', 'shadow', 'chunks', 'geometry'])
def test_launch_plan(program, case):
  out = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=120)
  assert out.returncode == 0, out.stderr[-3000:]
  assert out.stdout.strip() == case + ' ok'


def test_unknown_case_is_refused(program):
  assert subprocess.run([program, 'nothing'], stderr=subprocess.PIPE).returncode == 2
