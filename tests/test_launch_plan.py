"""Host-only check of the launch plan: which compiled form of each LM-round kernel a shard runs, and on what grid."""
import os
import subprocess

from conftest import ROOT


def test_launch_plan_pins_the_kernel_forms_of_each_shard(tmp_path):
    """Which compiled form of each LM-round kernel a shard runs, and on what grid, is decided in one place
    (csrc/launch_plan.hpp: makePlan). tests/host_cpp/launch_plan_check.cpp runs it on the HOST at 256 CUs for the
    benchmark's shards (c2, c3, c4 / c5 shards, c5 whole; fused, two-kernel and no-stream rounds) and for the knob routes
    the GPU tests take, against the forms the kernel profiles record."""
    exe = tmp_path / "launch_plan_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", "-w", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host_cpp", "launch_plan_check.cpp")], check=True, capture_output=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "20 plans, 0 mismatches" in out.stdout and out.stdout.rstrip().endswith("ok")
