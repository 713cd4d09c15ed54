"""The pair-of-3-vectors helpers of csrc/env_core.hpp (`v3p`: pk3, lo3, hi3, +, -, scalar *, the three cross products, the sym3 and rotation
products, pk6 / unpk6) against the scalar v3 helpers they replace, bit for bit -- no GPU needed.  tests/v3p_main.cpp is a stand-alone host
program over the host lane emulation (tests/host_emulation/lanes_cpu.hpp); it draws 4000 cases per helper itself: random mantissas with
exponents in -30 .. 30, one float in eight a signed zero (the product build compiles with -fno-signed-zeros, and so does this one), one in
eight at +-2^-30 or +-2^30, where every product and sum of a helper is still a normal finite number.  Three builds of the same text: the
product's floating-point flags; the same under the address and undefined-behaviour sanitizers, run as its own program; and -DIRRL_NO_V3P,
the A/B form in which the pair is two scalar v3."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc")
BUILDS = {"product_flags": ["-O1"], "sanitizers": ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover"], "no_v3p": ["-O1", "-DIRRL_NO_V3P"]}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_v3p_helper_equals_the_scalar_helper_bit_for_bit(build, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the host program"
    out = str(tmp_path / "v3p_main")
    subprocess.check_call([gxx, "-std=c++17", "-ffp-contract=on", "-fno-signed-zeros"] + BUILDS[build] +
                          ["-I" + CSRC, "-I" + os.path.join(ROOT, "tests", "host_emulation"), os.path.join(ROOT, "tests", "v3p_main.cpp"), "-o", out])
    res = subprocess.run([out, "1000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert res.returncode == 0, res.stdout
    assert "v3p: 48000 cases, all helpers bit for bit" in res.stdout, res.stdout
