"""Host-only check of the shard layout: the O(views) arithmetic of calib_set_problem."""
import os
import subprocess

from conftest import ROOT


def test_shard_layout_matches_a_brute_force_restatement(tmp_path):
    """The compact view list, the 512-point work items, the chunks of whole views, the views a 256-point tile spans and
    the uniform-shard test are computed in one place (csrc/shard_layout.hpp: makeShardLayout); they decide the LDS size
    of jacobian_kernel and every item table the kernels index. tests/host_cpp/shard_layout_check.cpp runs it on the HOST
    against a point-by-point restatement of each field: empty views, views of 512 / 513 / 1024 points, 300 one-point
    views in a tile, uniform shards and one with a shortened view, each at 1, 300 and 2^26 points per chunk, then 400
    seeded random offset vectors."""
    exe = tmp_path / "shard_layout_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", "-w", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host_cpp", "shard_layout_check.cpp")], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "442 cases, 0 mismatches" in out.stdout and out.stdout.rstrip().endswith("ok")
