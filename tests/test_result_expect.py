"""CPU side of the device-result tests: what the oracle makes of the chain-length inputs (so the
GPU cases reach the round counts they claim), and that the numpy path never imports torch."""
import subprocess
import sys

import numpy as np
import pytest

import result_expect as rx
from conftest import ROOT


@pytest.mark.parametrize("weighted", [False, True])
def test_chain_input_is_one_list_per_group(oracle, weighted):
    """One p_cluster(0.9) pass over the 2500 rows leaves exactly 15 rows whose member lists are
    the 15 groups, with exactly the planned sizes, and several lists not in ascending id order."""
    (rows, off, ids), want = rx.chain_reference(oracle, len(rx.CHAIN_SIZES), weighted)
    _, group = rx.chain_rows()
    assert rows.shape == (2500, rx.CHAIN_D)
    o_rows, o_off, o_ids = want
    assert o_rows.shape[0] == 15 and int(o_off[-1]) == ids.size
    row_of_id = np.empty(ids.size, np.int64)  # the input row that brought each id
    row_of_id[ids.astype(np.int64)] = np.repeat(np.arange(rows.shape[0]), np.diff(off.astype(np.int64)))
    sizes, unsorted = [], 0
    for i in range(15):
        lst = o_ids[int(o_off[i]):int(o_off[i + 1])].astype(np.int64)
        g = np.unique(group[row_of_id[lst]])
        assert g.size == 1, i
        assert np.unique(row_of_id[lst]).size == rx.CHAIN_SIZES[g[0]], i
        sizes.append(rx.CHAIN_SIZES[g[0]])
        unsorted += bool(np.any(np.diff(lst) < 0))
    assert sorted(sizes) == rx.CHAIN_SIZES
    assert unsorted >= 5
    if not weighted:
        assert rx.expected(want, ids)[3] == 11


def test_chain_prefixes_reach_every_round_count(oracle):
    """The prefixes of the size list used on the GPU: longest lists of 2, 3, 5, 9 and 1025 nodes,
    i.e. 1, 2, 3, 4 and 11 rounds — both buffer parities (no pass at all gives 0 rounds)."""
    got = []
    for n_groups in (2, 3, 5, 7, 15):
        (_, _, ids), want = rx.chain_reference(oracle, n_groups, False)
        assert int(np.diff(want[1].astype(np.int64)).max()) == rx.CHAIN_SIZES[n_groups - 1]
        got.append(rx.expected(want, ids)[3])
    assert got == [1, 2, 3, 4, 11]
    assert [rx.rounds(c) for c in (0, 1, 2, 3, 4, 5, 8, 9, 1024, 1025)] == [0, 0, 1, 2, 2, 3, 3, 4, 10, 11]


def test_numpy_path_does_not_import_torch():
    """`import kmerlsh_amd` and Engine.load_rows of a numpy array leave torch unimported (a fresh
    child process; the engine call itself is stubbed: no device is needed to take the numpy path)."""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import kmerlsh_amd
from kmerlsh_amd import _native
assert "torch" not in sys.modules, "import kmerlsh_amd imported torch"
calls = []
class Lib:
    def klsh_load_rows(self, ctx, rows, n, d, mo, mi):
        calls.append((n, d))
        return 0
eng = object.__new__(_native.Engine)
eng._ctx, eng._lib, eng.device, eng.d = None, Lib(), 0, 0
eng.load_rows(np.ones((5, 3), np.float32))
assert calls == [(5, 3)] and eng.d == 3
assert "torch" not in sys.modules, "load_rows of a numpy array imported torch"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
