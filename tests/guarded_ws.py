"""The guarded scratch allocator of the exact-workspace tests (test_workspace_exact_gpu.py, test_vccs_gpu.py)."""
import torch

DEV = 'cuda'
GUARD = 4096
FILL = 0xA5


class Guarded:
    """Stand-in for backend.workspace: [guard | nbytes | guard], all 0xA5; every buffer is kept until the test ends."""

    def __init__(self):
        self.bufs = []

    def __call__(self, nbytes, device=DEV):
        nbytes = int(nbytes)
        t = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.bufs.append((t, nbytes))
        return t[GUARD:GUARD + nbytes]

    def check(self):
        torch.cuda.synchronize()
        assert self.bufs, 'the builder never asked for scratch'
        for t, n in self.bufs:
            assert bool((t[:GUARD] == FILL).all()), 'the guard below %d bytes of scratch was written' % n
            assert bool((t[GUARD + n:] == FILL).all()), 'the guard above %d bytes of scratch was written' % n
