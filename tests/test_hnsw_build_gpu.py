"""mevi_graph_link (csrc/graph_build.hip) against tests/graph_cases.py: link_expected.  The output is exactly determined by the
lists: equality of every slot, whatever the workspace."""
import numpy as np
import pytest
import torch

import graph_cases as gc
from mevi_amd import dense

pytestmark = pytest.mark.gpu


def _lists(seed, nd, C, hub=False):
    rng = np.random.default_rng(seed)
    knn = rng.integers(-1, nd, size=(nd, C))
    knn[:, 0] = np.arange(nd)                                          # the row itself, as a search of the rows returns it
    if C > 4:
        knn[::3, 4] = knn[::3, 2]                                      # repeats
        knn[::11, 3] = nd + 5                                          # past the end
    if hub:
        knn[1:, min(1, C - 1)] = 0                                     # row 0 is the first other row of every list
    return knn.astype(np.int64)


def _link(cuda, knn, M, workspace_bytes=None):
    t = torch.from_numpy(knn).to(cuda)
    ws = None if workspace_bytes is None else torch.empty(workspace_bytes, dtype=torch.uint8, device=cuda)
    g = dense.graph_link(t, M, workspace=ws)
    torch.cuda.synchronize()
    return g.cpu().numpy()


@pytest.mark.parametrize("nd,C,M,hub", [(3000, 17, 16, False), (3000, 9, 16, False), (3000, 40, 8, False), (5000, 5, 2, True),
                                        (9000, 6, 4, True), (700, 300, 256, False), (1, 3, 2, False)],
                         ids=["C_is_M_plus_1", "C_below_M", "C_above_M", "hub_M2", "hub_M4_two_ranges", "M256", "one_row"])
def test_link_equals_the_reference_whatever_the_workspace(cuda, nd, C, M, hub):
    knn = _lists(nd * 31 + C, nd, C, hub)
    want = gc.link_expected(knn, M)
    if hub:
        assert (want[0] >= 0).all() and (np.array([(row == 0).any() for row in want[1:]])).all()     # in-degree nd - 1
    least = dense.graph_link_workspace_bytes(nd, C, M)
    assert least == -(-min(nd, dense.GRAPH_LINK_MIN_ROWS) * 2 * M * 8 // 256) * 256
    np.testing.assert_array_equal(_link(cuda, knn, M, least), want)                    # nd > 4096: more than one destination range
    np.testing.assert_array_equal(_link(cuda, knn, M, least + 2 * M * 8 * 700 + 256), want)     # ranges of another size
    np.testing.assert_array_equal(_link(cuda, knn, M), want)                           # generous: one range
