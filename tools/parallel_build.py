"""`__graft_entry__.build()` with the per-model hipcc runs spread over the host
cores: the specs `build()` would realise are recorded first (`build.realise`
replaced by a recorder), then realised in a process pool, then `build()` itself
runs (everything is cached by then, so it only verifies)."""
import multiprocessing as mp
import os
import sys
import time
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _one(spec):
  from dm_control_amd import build
  try:
    build.realise(spec)
    return None
  except Exception as e:  # pylint: disable=broad-except
    return '%r: %s' % (spec[1:7], str(e)[-300:])


def main():
  import __graft_entry__ as entry
  from dm_control_amd import build
  jobs = []

  def record(spec, force=False, keep_temps=False):
    jobs.append(spec)
    return 'recorded'
  with mock.patch.object(build, 'realise', record):
    entry.build()
  workers = int(sys.argv[1]) if len(sys.argv) > 1 else max(1, (os.cpu_count() or 2) - 1)
  t0 = time.time()
  with mp.get_context('fork').Pool(workers) as pool:
    for err in pool.imap_unordered(_one, jobs):
      if err:
        print('FAILED', err, flush=True)
  print('%d builds in %.0f s on %d workers' % (len(jobs), time.time() - t0, workers),
        flush=True)
  entry.build()
  print('build() ok', flush=True)


if __name__ == '__main__':
  main()
