"""stfem_neighbour_exchange (the transport of the CIP ghost planes between z-slabs) on ONE GPU: the one-rank communicator whose lower
and upper neighbour are the rank itself (tests/test_gpu_comm.py).  What is sent up arrives in recv_below, what is sent down in
recv_above, bit for bit; a side with rank -1 is skipped and its buffers are not touched."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_self_loop_neighbour_exchange():
    stfem = importlib.import_module("dealii-stfem_amd")
    dmod = importlib.import_module("dealii-stfem_amd.distributed")
    if not stfem.lib().stfem_comm_available():
        pytest.skip("no RCCL in this process")
    op = stfem.StokesMatrixFreeOperator((3, 2, 2))
    count = op.cip_ghost_size  # 6 * 7 * 5 = 210 doubles of 3 * 175
    size = 3 * op.n_velocity
    assert 0 < count < size
    rng = np.random.default_rng(3)
    DOWN, UP, FILL = rng.uniform(-1, 1, size), rng.uniform(-1, 1, size), np.full(size, 5.0)
    down, up = op.initialize_dof_vector(0, DOWN), op.initialize_dof_vector(0, UP)
    comm = dmod.Communicator(0, 1, 0, lambda raw: raw)

    below, above = op.initialize_dof_vector(0, FILL), op.initialize_dof_vector(0, FILL)
    comm.neighbour_exchange(0, 0, count, down, up, below, above)
    B, A = below.download(), above.download()  # (a synchronous copy on the null stream, on which the exchange was ordered)
    assert np.array_equal(B[:count], UP[:count]) and np.array_equal(A[:count], DOWN[:count])
    assert np.array_equal(B[count:], FILL[count:]) and np.array_equal(A[count:], FILL[count:])
    assert np.array_equal(down.download(), DOWN) and np.array_equal(up.download(), UP)

    # no lower neighbour: the lower side's buffers are not touched (and may be absent); no neighbour at all: nothing moves
    below, above = op.initialize_dof_vector(0, FILL), op.initialize_dof_vector(0, FILL)
    comm.neighbour_exchange(-1, 0, count, down, up, below, above)
    assert np.array_equal(below.download(), FILL)
    assert np.array_equal(above.download()[:count], UP[:count])  # (the self-loop's only receive meets its only send)
    above = op.initialize_dof_vector(0, FILL)
    comm.neighbour_exchange(-1, 0, count, None, up, None, above)
    assert np.array_equal(above.download()[:count], UP[:count])
    comm.neighbour_exchange(-1, -1, count, None, None, None, None)

    # refusals: a rank that does not exist, a missing buffer of a side that is named
    with pytest.raises(RuntimeError):
        comm.neighbour_exchange(0, 1, count, down, up, below, above)
    with pytest.raises(RuntimeError):
        comm.neighbour_exchange(0, 0, count, down, up, None, above)
    comm.close()
