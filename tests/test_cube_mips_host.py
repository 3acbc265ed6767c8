"""csrc/cube_mips_core.hpp on the host (tests/cube_mips_host): the kernel body's chain equals geometry.cube_mip_chain byte for byte,
at the sizes the GPU tier uses, and touches nothing past it."""
import numpy as np
import pytest

import cube_mips_host_lib


@pytest.mark.parametrize("dim", [1, 2, 3, 5, 64, 65, 96, 130, 200, 256])
def test_host_body_equals_the_definition(built_lib, dim):
    from crychic_renderer_amd import geometry as g
    cube = np.random.default_rng(dim).integers(0, 256, (6, dim, dim, 4), dtype=np.uint8)
    ref, levels = g.cube_mip_chain(cube)
    got, n = cube_mips_host_lib.generate(cube, levels)
    assert n == ref.size and np.array_equal(got[:n], ref)
    assert (got[n:] == 0xA5).all()


def test_host_body_dword_path_and_capped_levels(built_lib):
    """A chain that is not 16-byte aligned takes the dword loads; a capped chain stops at its last level."""
    from crychic_renderer_amd import geometry as g
    cube = np.random.default_rng(9).integers(0, 256, (6, 96, 96, 4), dtype=np.uint8)
    ref, levels = g.cube_mip_chain(cube, 3)
    got, n = cube_mips_host_lib.generate(cube, 3, misalign=4)
    assert levels == 3 and np.array_equal(got[:n], ref) and (got[n:] == 0xA5).all()
