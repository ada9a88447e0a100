"""The one build of gss_run on the CPU fakes (tests/helpers: fake_hip, fake_dev.cpp) for the tests
that drive it with a program of tests/helpers (run_fake.cpp, impair_fake.cpp, jam_fake.cpp,
echo_fake.cpp, fir_fake.cpp).  What does not depend on the program (the host plane, cli_args,
gss_run.hip, gss_run_plan.hip and gss_run_pool.hip compiled as C++, fake_hip and fake_dev) is
compiled once per pytest session and kept here; a program adds its own object, and its
-DNO_LAUNCH twin where it has one."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(REPO, "tests", "helpers")
CF = ["-O2", "-g", "-ffp-contract=off", "-fno-fast-math", "-D_FILE_OFFSET_BITS=64",
      "-I" + os.path.join(REPO, "include")]
INC = ["-I" + HELPERS, "-I" + os.path.join(HELPERS, "fake_hip")]

_common = None      # (directory, objects)


def _cxx(src, obj, extra=()):
    subprocess.run(["g++", "-std=c++17"] + CF + INC + list(extra) + ["-c", src, "-o", obj],
                   check=True)


def common_objects(tmp_path_factory):
    global _common
    if _common is None:
        d = str(tmp_path_factory.mktemp("fake"))
        csrc = os.path.join(REPO, "gps-sdr-sim_amd", "csrc")
        host = os.path.join(csrc, "host")
        srcs = [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith(".c")]
        srcs.append(os.path.join(csrc, "cli", "cli_args.c"))
        objs = []
        for s in srcs:
            objs.append(os.path.join(d, os.path.basename(s)[:-2] + ".o"))
            subprocess.run(["gcc"] + CF + ["-c", s, "-o", objs[-1]], check=True)
        # the driver's three translation units, each compiled on its own as the library's are
        # (GSS_RUN_SEPARATE: gss_run.hip alone would take the other two in)
        hip_cxx = ["-x", "c++", "-DGSS_RUN_SEPARATE"]
        for s, extra in ((os.path.join(csrc, "hip", "gss_run.hip"), hip_cxx),
                         (os.path.join(csrc, "hip", "gss_run_plan.hip"), hip_cxx),
                         (os.path.join(csrc, "hip", "gss_run_pool.hip"), hip_cxx),
                         (os.path.join(HELPERS, "fake_hip", "fake_hip.cpp"), []),
                         (os.path.join(HELPERS, "fake_dev.cpp"), [])):
            objs.append(os.path.join(d, os.path.basename(s).rsplit(".", 1)[0] + ".o"))
            _cxx(s, objs[-1], extra)
        _common = (d, objs)
    return _common


def programs(tmp_path_factory, name, nolaunch=True):
    """{name: executable, name + "_nolaunch": executable} of tests/helpers/<name>.cpp"""
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("gcc/g++ not available")
    d, objs = common_objects(tmp_path_factory)
    exes = {}
    for tag, defs in ((name, []), (name + "_nolaunch", ["-DNO_LAUNCH"]))[:2 if nolaunch else 1]:
        o = os.path.join(d, tag + ".o")
        _cxx(os.path.join(HELPERS, name + ".cpp"), o, defs)
        exes[tag] = os.path.join(d, tag)
        subprocess.run(["g++", "-o", exes[tag]] + objs + [o, "-lm", "-lpthread"], check=True)
    return exes
