"""Host-only check of the block maps: where each solver on the shared LM loop keeps its normal equations."""
import os
import subprocess

from conftest import ROOT


def test_block_maps_match_a_restatement_of_the_record_tables(tmp_path):
    """The four *_normal_eq entry points read (totals, view records) through one unpack_blocks and one BlockMap per layout
    (csrc/block_map.hpp: kSt*, JointLayout, RigLayout, RigJointDesc). tests/host_cpp/block_map_check.cpp runs them on the
    HOST: totals and three view records whose values name their own slot, unpacked and compared entry by entry -- B
    symmetric and an exact zero outside its blocks, E, V, g, the per-camera errors -- with the record tables of DESIGN.md
    written out again: the stereo solver, joint stereo at the four model pairs, the rig at N = 2, 3, 8, the joint rig at
    every model mix of N = 2 and 3 and four of N = 8, eight radtan cameras (S = 122) among them."""
    exe = tmp_path / "block_map_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", "-w", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host_cpp", "block_map_check.cpp")], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "24 cases, 0 mismatches" in out.stdout and out.stdout.rstrip().endswith("ok")
