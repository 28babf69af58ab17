"""Host arithmetic only: the constructions of tests/test_dense_workspace_gpu.py really force the paths that file names."""
import numpy as np

from tests.test_dense_workspace_gpu import _case


def test_the_constructions_put_their_duplicates_across_rank_k():
    """The near-copies are query 0's best rows, in one block followed by a gap, and more of them than the survivor lists hold."""
    for name, copies in (("250 near-copies", 250), ("5000 near-copies", 5000)):
        q, d, k = _case(name)
        s = np.sort(d @ q[0])[::-1]
        assert s[copies - 1] - s[copies] > 1e3 * (s[0] - s[copies - 1]) and k < copies, name
    q, d, k = _case("50 distinct rows")
    s = np.sort(d @ q[0])[::-1]
    assert s[0] == s[k] == s[3 * k + 64]                                 # ties run past the 8-bit pass's 3 k + 64 survivors
    q, d, k = _case("sorted rows")
    assert (np.argsort(-(d @ q[:6].T), axis=0)[:k] > len(d) - 1000).all()   # the best rows come last
