"""CPU-side checks of the workspace sizes that need no field handle.  Every size in the library is its layout run on a null base
(csrc/workspace.h), so a size pins a layout: the presample's, the renderer's and the occupancy refresh's are held to the byte, and the
two scoring sizes (csrc/score.hip), once a closed formula with slack, to "positive and no larger than the formula gave"."""
import pytest

import apnrf_amd


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    return apnrf_amd.load_library()


PRESAMPLE = [      # (n_rays, max_marched) -> bytes; 65536 / 65537 lie on either side of the scratch-row clamp, 2097153 at its floor of 64
    ((1, 1), 20736), ((100, 1000), 1660416), ((2000, 262144), 37013504), ((65536, 1048576), 1092094720), ((65537, 1048576), 1091587840),
    ((2097153, 4194304), 1191194624), ((0, 5), -1), ((5, 0), -1),
]
RENDER = [         # (n_rays, rays_per_view) -> bytes
    ((1, 1), 72448), ((64, 64), 77824), ((192, 64), 94208), ((4096, 4096), 557568), ((12288, 4096), 1534464), ((5000, 1000), 666624),
    ((409600, 409600), 48915456), ((0, 1), -1),
]
OCC = [            # (cells_per_level, fused) -> bytes
    ((1, 0), 4608), ((1, 1), 5376), ((1000, 1), 32768), ((2097152, 0), 8654848), ((2097152, 1), 58986496), ((0, 1), -1),
]
SCORE = [          # (members, views, pixels, classes) -> what the closed formulas gave: (poses, trajectory)
    ((1, 1, 1, 1), (79744, 78992)), ((1, 1, 64, 29), (96320, 94560)), ((2, 3, 64, 29), (401152, 393312)), ((1, 3, 64, 29), (275136, 271392)),
    ((1, 5, 64, 29), (384000, 378272)), ((3, 7, 100, 1), (587136, 550944)), ((4, 5, 81, 40), (830792, 801192)), ((16, 2, 64, 3), (1524224, 1475392)),
    ((2, 32, 4096, 29), (74540288, 70360576)), ((2, 256, 4096, 29), (594321664, 560896512)),
]


@pytest.mark.parametrize("args,want", PRESAMPLE)
def test_presample_workspace_bytes(lib, args, want):
    assert lib.mnf_train_presample_workspace_bytes(*args) == want


@pytest.mark.parametrize("args,want", RENDER)
def test_render_workspace_bytes(lib, args, want):
    assert lib.mnf_render_workspace_bytes(*args) == want


@pytest.mark.parametrize("args,want", OCC)
def test_occ_workspace_bytes(lib, args, want):
    assert lib.mnf_occ_workspace_bytes(*args) == want


@pytest.mark.parametrize("args,cap", SCORE)
def test_score_workspace_bytes_positive_and_capped(lib, args, cap):
    poses, traj = lib.mnf_score_poses_workspace_bytes(*args), lib.mnf_score_trajectory_workspace_bytes(*args)
    assert 0 < poses <= cap[0]
    assert 0 < traj <= cap[1]


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("bad", [0, -1])
def test_score_workspace_bytes_refuse_non_positive(lib, k, bad):
    args = [2, 3, 64, 29]
    args[k] = bad
    assert lib.mnf_score_poses_workspace_bytes(*args) == -1
    assert lib.mnf_score_trajectory_workspace_bytes(*args) == -1
