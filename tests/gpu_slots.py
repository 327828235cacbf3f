"""GPU process slots for one test session (TEST INFRASTRUCTURE: imported by tests/ and tests/oracle_farm.py only).

A shared MI355X box allows at most MAX_GPU_PROCESSES processes with the GPU open at once.  The pytest process is one of them;
everything the tests start besides it -- data-parallel ranks, bench.py runs, the oracle farm's gradient workers -- draws from the
remaining SLOTS.  A process opens the GPU more often than it seems: torch's autograd engine asks every device backend for its
device count on its FIRST backward, so even a pure host (fp64 CPU) oracle backward opens /dev/kfd, whatever HIP_VISIBLE_DEVICES
says.

The slots are lock files under one directory per session (LU_GPU_SLOT_DIR, inherited by child processes).  flock() locks die
with the process that holds them, so a killed worker never leaks a slot.  A gate lock makes every acquisition of several slots
atomic: a test that needs five waits for the farm workers running at the time, and is not overtaken by the ones queued after it."""
import contextlib
import fcntl
import os
import tempfile
import time

MAX_GPU_PROCESSES = 6
SLOTS = MAX_GPU_PROCESSES - 1      # the pytest process holds the GPU itself


def slot_dir():
    d = os.environ.get('LU_GPU_SLOT_DIR')
    if not d:
        d = os.environ['LU_GPU_SLOT_DIR'] = tempfile.mkdtemp(prefix='lu_gpu_slots_')
    return d


def acquire(n):
    """Block until n slots are held by this process; returns the open lock files (closing them releases the slots)."""
    assert 1 <= n <= SLOTS, 'a test may start at most %d GPU processes besides pytest, not %d' % (SLOTS, n)
    d = slot_dir()
    held = []
    with open(os.path.join(d, 'gate'), 'a+') as gate:
        fcntl.flock(gate, fcntl.LOCK_EX)
        try:
            while len(held) < n:
                for i in range(SLOTS):
                    if len(held) == n:
                        break
                    f = open(os.path.join(d, 'slot%d' % i), 'a+')
                    try:
                        fcntl.flock(f, fcntl.LOCK_EX | fcntl.LOCK_NB)
                    except OSError:
                        f.close()      # held by another process (or already by this one)
                        continue
                    held.append(f)
                if len(held) < n:
                    time.sleep(0.2)
        finally:
            fcntl.flock(gate, fcntl.LOCK_UN)
    return held


@contextlib.contextmanager
def hold(n):
    """`with hold(n):` around starting n GPU-using processes AND waiting for them to end."""
    held = acquire(n)
    try:
        yield
    finally:
        for f in held:
            f.close()
