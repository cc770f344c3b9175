"""The table of grid_wrap_ref64.py held to the launch arithmetic it restates and to the grid_for(...) lines of the sources: every row
reaches the arm it names, every new row is minimal (nobody quietly grows the cases), and a launcher whose work expression changes
fails here instead of leaving the table stale.  No GPU."""
import pytest

import grid_wrap_ref64 as W

IDS = [c[0] for c in W.CASES]


def test_grid_for_is_the_helper_of_host_common():
    assert [W.grid_for(w) for w in (0, 1, 256, 257, W.T, W.T + 1, 10 ** 9)] == [1, 1, 1, 2, 2048, 2048, 2048]
    assert W.grid_for(W.T4 + 1, 256, 4096) == 4096 and W.grid_for(W.T4 - 256, 256, 4096) == 4095
    # the signature's defaults, as host_common.h writes them
    with open(W.os.path.join(W.CSRC, 'host_common.h')) as f:
        assert 'inline int grid_for(size_t work, int per_block = 256, int cap = 2048)' in f.read()
    assert W.resident_threads() == W.PER_BLOCK               # rows_narrow_kernel's THREADS: stride() counts 256 threads per workgroup


@pytest.mark.parametrize('cid', IDS)
def test_row_reaches_the_arm_it_names(cid):
    _, name, shape, arm, _ = W.case(cid)
    assert W.arm(name, shape) == arm, (cid, W.arm(name, shape))
    assert W.trips(name, shape) >= 2
    assert W.stride(name, shape) == (W.T4 if W.LAUNCHERS[name][3] == W.CAP4 else W.T)        # the launch sits at its cap
    if 'q1 live and dead' in arm:                            # both outcomes of `two` occur in trip 2
        threads, live, dead = W.last_trip(name, shape)
        assert live > 0 and dead > 0 and live + dead == threads


@pytest.mark.parametrize('cid', [i for i in IDS if i not in W.EXISTING])
def test_new_rows_are_minimal(cid):
    _, name, shape, arm, _ = W.case(cid)
    over = W.items(name, shape) - W.threshold(name, shape, arm)
    assert 0 < over <= W.MINIMAL, (cid, over)


def test_the_issue_counts():
    """the shapes the optimizer cases were specified with"""
    assert W.ADAM2_COUNT == 6292656 and W.ADAM2_COUNT % 4 == 0
    assert W.last_trip('adam2_kernel', dict(count=W.ADAM2_COUNT)) == (W.T, 300, W.T - 300)
    assert W.ADAM_TAIL_COUNT % 4 == 3
    head, quads, scalars = W._optim_split(W.OPT_ALIGNED)
    assert (head, quads, scalars) == (3, 3 * W.T + 300, 5)
    assert W.last_trip('optim_kernel', W.OPT_ALIGNED) == (W.T, 300, W.T - 300)
    assert W._optim_split(dict(n=W.T + 300, offs=W.OPT_MIXED)) == (W.T + 300, 0, W.T + 300)       # scalar throughout
    assert W._optim_split(dict(n=W.T + 300, offs=W.OPT_MIXED[:3])) == (W.T + 300, 0, W.T + 300)   # the one-state rules: three buffers
    for n, offs in W.OPTIM_SCALAR_SINGLE:
        s = dict(n=n, offs=offs)
        assert W._optim_split(s) == (n, 0, n) and W.trips('optim_kernel scalars', s) == 1
    # below its threshold every row falls back to one trip: what the minimality assertion guards
    assert W.arm('adam2_kernel', dict(count=4 * 2 * W.T)) == 'trip 1'
    assert W.arm('adam2_kernel', dict(count=4 * 3 * W.T)) == 'trip 2, q1 dead'
    assert W.arm('glu_fwd', dict(M=W.GLU_M - 16, R=W.GLU_R)) == 'trip 1'
    # rows_narrow: a destination one element past a 16-byte boundary has a scalar head of 7, and the 16-byte stores start behind it
    s = W.shape_of('rows_narrow head')
    assert W.items('rows_narrow', s) == W.T + 300 and (s['count'] - 7) % 8 == 3
    assert W.arm('rows_narrow', dict(count=8 * W.T + 7, dst_off=0)) == 'trip 1'


def test_every_launcher_has_a_row():
    """a launcher held to the source is also run by some row (the two optim rows share one kernel)"""
    assert {c[1] for c in W.CASES} == set(W.LAUNCHERS)


@pytest.mark.parametrize('name', sorted(W.LAUNCHERS))
def test_sources_still_launch_with_the_restated_work(name):
    """the argument text of the kernel's grid_for( calls, as the .hip file writes it"""
    want = W.LAUNCHERS[name][2]
    got = W.source_args(name)
    assert got, (name, 'no grid_for( line names this kernel')
    assert all(a == want for a in got), (name, got, want)
