"""The auto-invalidation timers on the device (fgi_timers_auto_open and its calls, C-ABI 0.13) against the model of
test_auto_timers_model.py.

Every scenario there is driven on the engine and on the CPU oracle + model together; after every step the engine
must equal the model in the returned id set, fgi_dump_states over every handle, fgi_timers_list and
fgi_timers_list_ex (kinds included), the fired count, fgi_timers_next_due, the statistics (armed == fired +
dropped + stored) and the auto statistics. The gates at the end check what the model does not cover: the status
codes, fgi_restore, fgi_timers_close, partitions and the inertness of a graph that never opens auto."""
import numpy as np
import pytest

from harness import build_pair
from test_gpu_flagged import _engine
from test_gpu_part_mutations import _group
from test_gpu_stream import _mix
import test_auto_timers_model as A

pytestmark = pytest.mark.gpu

ZERO = dict(armed_auto=0, merged=0, fired_auto=0)


def _maker(pkg, labels=-1):
    def make(arrays, n_det, **kw):
        g = _engine(pkg, len(arrays[0]), *arrays, labels=labels, n_detached=n_det)
        return A.AutoDriver(arrays, n_det, engine=g, fgi=pkg.fgi, **kw)
    return make


def test_chain(pkg, gpu_available):
    drv = A.scn_chain(_maker(pkg))
    assert drv.g.timers_auto_stats() == dict(armed_auto=1, merged=0, fired_auto=1)


@pytest.mark.parametrize("labels", [-1, 1])
def test_selection(pkg, gpu_available, labels):
    A.scn_selection(_maker(pkg, labels))
    A.scn_no_defaults(_maker(pkg, labels))


def test_ioso_with_a_delay_gets_its_delay_entry_only(pkg, gpu_available):
    drv = A.scn_ioso_delay(_maker(pkg))
    assert list(drv.g.timers_list_ex()[3]) == []


@pytest.mark.parametrize("labels", [-1, 1])
def test_merge_both_directions(pkg, gpu_available, labels):
    assert A.scn_merge(_maker(pkg, labels)).ca["merged"] == 3
    assert A.scn_delay_then_auto(_maker(pkg, labels)).ca["merged"] == 1


@pytest.mark.parametrize("labels", [-1, 1])
def test_displacement(pkg, gpu_available, labels):
    A.scn_displacement(_maker(pkg, labels))


def test_batch(pkg, gpu_available):
    A.scn_batch(_maker(pkg))


def test_cascading(pkg, gpu_available):
    A.scn_cascading(_maker(pkg))


@pytest.mark.parametrize("labels", [-1, 1])
def test_start_auto_on_bulk_registered_nodes(pkg, gpu_available, labels):
    A.scn_start_auto(_maker(pkg, labels))


@pytest.mark.parametrize("labels", [-1, 1])
def test_past_one_grid(pkg, gpu_available, labels):
    """k_tm_arm_auto on its second trip, from start_auto and from set_output (test_past_one_grid_model states the
    sizes)."""
    drv = A.scn_past_one_grid(_maker(pkg, labels))
    assert drv.g.timers_stats()["runs"] == 2


def test_computed_options(pkg, gpu_available):
    """AnonymousComputedTest.ComputedOptionsTest with the tick firing, not a hand-made invalidation."""
    drv, values = A.scn_computed_options(_maker(pkg))
    assert values == 4 and drv.g.timers_auto_stats()["fired_auto"] == 3


# ---- gates ---------------------------------------------------------------------------------------------------

def _begun(pkg, n=4, n_det=0):
    """n empty slots, every one begun (Computing)."""
    g = _engine(pkg, n, *A.slot_arrays(n), n_detached=n_det)
    g.begin_compute(np.arange(n, dtype=np.uint32), 10 + np.arange(n, dtype=np.uint64))
    return g


def _raises(pkg, status, call):
    with pytest.raises(pkg.FgiError) as e:
        call()
    assert e.value.status == status, e.value


def test_status_gates(pkg, gpu_available):
    fgi = pkg.fgi
    g = _begun(pkg)
    assert g.timers_auto_stats() == ZERO
    calls = (g.timers_auto_open, lambda: g.timers_set_auto_delay([0], [5]), lambda: g.timers_start_auto([0]),
             g.timers_list_ex)
    for call in calls:
        _raises(pkg, fgi.ESTATE, call)                   # before fgi_timers_open
    g.timers_open()
    for call in calls[1:3]:
        _raises(pkg, fgi.ESTATE, call)                   # timers open, auto not
    assert [len(a) for a in g.timers_list_ex()] == [0, 0, 0, 0]
    g.timers_auto_open(default_auto=4)
    _raises(pkg, fgi.ESTATE, g.timers_auto_open)         # a second open
    # a handle out of range, or listed twice: nothing stored
    _raises(pkg, fgi.EINVAL, lambda: g.timers_set_auto_delay([1, 4], [5, 5]))
    _raises(pkg, fgi.EINVAL, lambda: g.timers_set_auto_delay([1, 1], [5, 6]))
    g.set_output([0, 1])
    assert list(g.timers_list_ex()[2]) == [4, 4]         # slot 1 kept the default: the refused calls stored no delay
    _raises(pkg, fgi.EINVAL, lambda: g.timers_start_auto([2, 9]))
    _raises(pkg, fgi.EINVAL, lambda: g.timers_start_auto([0, 0]))
    assert g.timers_stats()["stored"] == 2 and g.timers_auto_stats() == dict(armed_auto=2, merged=0, fired_auto=0)


def test_restore_drops_entries_and_keeps_delays(pkg, gpu_available):
    g = _begun(pkg)
    g.timers_open(now=3)
    g.timers_auto_open()
    g.timers_set_auto_delay([0, 1], [5, 0], [0, 7])
    g.snapshot()
    g.set_output([0, 1], transient=[0, 1])
    assert [list(a) for a in g.timers_list_ex()[::2]] == [[0, 1], [8, 10]]
    g.restore()
    st = g.timers_stats()
    assert st["stored"] == 0 and st["dropped"] == 2 and st["armed"] == 2 and len(g.timers_list_ex()[0]) == 0
    g.set_output([0, 1], transient=[0, 1])               # the clock and the delays stayed
    assert [list(a) for a in g.timers_list_ex()[::2]] == [[0, 1], [8, 10]]
    assert list(g.timers_list_ex()[3]) == [1, 1]


def test_close_turns_auto_off(pkg, gpu_available):
    fgi = pkg.fgi
    g = _begun(pkg)
    g.timers_open()
    g.timers_auto_open(default_auto=4)
    g.set_output([0])
    assert g.timers_stats()["stored"] == 1
    g.timers_close()
    assert g.timers_auto_stats() == ZERO
    g.set_output([1])                                    # arms nothing
    _raises(pkg, fgi.ESTATE, g.timers_list_ex)
    g.timers_open()
    g.set_output([2])                                    # timers open again, auto not
    assert g.timers_stats()["armed"] == 0 and g.timers_auto_stats() == ZERO
    _raises(pkg, fgi.ESTATE, lambda: g.timers_start_auto([2]))
    g.timers_auto_open(default_auto=4)
    g.timers_start_auto([0, 1, 2, 3])                    # 3 is still Computing
    assert list(g.timers_list_ex()[0]) == [0, 1, 2]


def test_a_graph_that_never_opens_auto_is_inert(pkg, gpu_available):
    """Timers open, auto never: set_output (plain, with transient flags, and as a batch's step with flags) leaves
    the timers' statistics and list as they are, and the auto statistics are zero."""
    g = _engine(pkg, 6, *A.slot_arrays(6, consistent=[0], delayed=[1], edges=[(0, 1)]), n_detached=0)
    g.timers_open(default_delay=5)
    g.invalidate([0])
    stats, listed = g.timers_stats(), [list(a) for a in g.timers_list()]
    assert stats["stored"] == 1
    g.begin_compute([2, 3, 4], [7, 8, 9])
    out, _ = g.set_output([2])
    assert list(out) == [1]
    out, _ = g.set_output([3], transient=[1])
    assert list(out) == [1]
    _, outs = g.run_batch([("set_output", [4], [1])])
    assert list(outs[0]) == [1]
    after = g.timers_stats()
    for k in ("stored", "armed", "fired", "dropped", "moved", "runs"):
        assert after[k] == stats[k], k
    assert [list(a) for a in g.timers_list()] == listed
    assert g.timers_auto_stats() == ZERO and list(g.timers_list_ex()[3]) == [0]


def test_a_poisoned_graph_is_refused(pkg, gpu_available):
    """Every call of the section on a poisoned graph: FGI_ESTATE. Poisoned as test_gpu_batch.py's
    test_restore_without_snapshot_keeps_the_graph_poisoned does it (FGI_OPT_FAULT_INJECT: a block leaves a cascade's
    grid barrier without arriving, the batch returns FGI_EDEVICE)."""
    fgi = pkg.fgi
    mix = _mix(pkg, 8, 50, 2, 0, 0x5EED00E0)
    used, dep, tag = mix.initial_edges()
    g, o = build_pair(pkg, mix.n, mix.version.copy(), mix.state_flags(), used, dep, tag)
    o.close()
    g.timers_open()
    g.set_option(fgi.OPT_FAULT_INJECT, 1)
    _raises(pkg, fgi.EDEVICE, lambda: g.run_batch([("invalidate", mix.roots(0))]))
    for call in (g.timers_auto_open, lambda: g.timers_set_auto_delay([0], [5]), lambda: g.timers_start_auto([0]),
                 g.timers_list_ex, lambda: g.set_output([0], transient=[0])):
        _raises(pkg, fgi.ESTATE, call)
    g.close()


def test_partition_rank_is_refused(pkg, gpu_available):
    fgi = pkg.fgi
    gs, _ = _group(pkg, 2, 64)
    for g in gs:
        for call in (g.timers_auto_open, lambda: g.timers_set_auto_delay([0], [5]), lambda: g.timers_start_auto([0]),
                     g.timers_auto_stats, g.timers_list_ex):
            _raises(pkg, fgi.ENOTSUP, call)
        h = np.zeros(1, np.uint32)
        t = np.zeros(1, np.uint8)
        st = g.lib.fgi_set_output_ex(g.h, 1, h.ctypes.data_as(fgi._u32p), t.ctypes.data_as(fgi._u8p), None, None, 0, None, None)
        assert st == fgi.ENOTSUP
