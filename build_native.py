#!/usr/bin/env python3
"""Build the native parts of wormhole_amd in-tree (gfx950 only).

Two shared objects are produced next to the Python sources:

* ``wormhole_amd/_hip.so``  -- hand-written CDNA4 HIP kernels (``csrc/hip/*.hip``,
  compiled by ``hipcc --offload-arch=gfx950`` WITHOUT torch headers so each
  kernel file builds in seconds) plus the torch/pybind11 binding layer
  (``csrc/bind/*.cc``, host-only g++ compile that validates tensors and
  launches on the current HIP stream).
* ``bin/native/{convert,text2crb}`` -- standalone C++ data conversion tools
  (reference learn/tool/), wrapped by ``bin/convert.dmlc`` / ``bin/text2crb.dmlc``.
* ``bin/native/{host_selftest,gbdt_rank_plan_test,gbdt_shap_plan_test,
  gbdt_shap_inter_test,gbdt_dart_plan_test,gbdt_quantile_plan_test,
  gbdt_leaf_plan_test,gbdt_survival_plan_test}`` --
  stand-alone tests of host code (``--sanitize`` / ``--sanitize-rank-plan`` /
  ``--sanitize-shap-plan`` / ``--sanitize-shap-inter`` / ``--sanitize-dart-plan``
  / ``--sanitize-quantile-plan`` / ``--sanitize-leaf-plan`` /
  ``--sanitize-survival-plan`` build them under sanitizers).
* ``wormhole_amd/_host.so`` -- the native C++ runtime (``csrc/host/*.cc``):
  proto-text config parser, data parsers (libsvm / criteo / adfea / crb),
  CityHash64, LZ4 block codec, RecordIO, workload pool, control-plane
  sockets, CPU localizer.  Host-only, no GPU needed.

A ``build/build.ninja`` is generated and driven by ninja so rebuilds are
incremental and parallel.  Usage: ``python build_native.py [-j N] [--clean]``.
"""
import argparse
import glob
import os
import shutil
import subprocess
import sys
import sysconfig

ROOT = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(ROOT, "build")
PKG = os.path.join(ROOT, "wormhole_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = "gfx950"


def torch_paths():
    import torch
    from torch.utils import cpp_extension as ce
    inc = ce.include_paths()
    lib = ce.library_paths()[0]
    abi = int(torch._C._GLIBCXX_USE_CXX11_ABI)
    return inc, lib, abi


def gen_ninja():
    inc, tlib, abi = torch_paths()
    pyinc = sysconfig.get_paths()["include"]
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    common_inc = "-I%s/csrc" % ROOT
    tinc = " ".join("-isystem %s" % p for p in inc) + " -isystem %s" % pyinc
    cxxflags = ("-O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-sign-compare "
                "-D_GLIBCXX_USE_CXX11_ABI=%d %s" % (abi, common_inc))
    hipflags = ("-O3 -std=c++17 -fPIC --offload-arch=%s -munsafe-fp-atomics "
                "-Wno-unused-result %s" % (ARCH, common_inc))
    bindflags = ("%s -D__HIP_PLATFORM_AMD__ -DUSE_ROCM -isystem %s/include %s "
                 "-DTORCH_API_INCLUDE_EXTENSION_H" % (cxxflags, ROCM, tinc))
    hostflags = "%s %s -DTORCH_API_INCLUDE_EXTENSION_H -pthread" % (cxxflags, tinc)
    tlibs = "-L%s -Wl,-rpath,%s -lc10 -ltorch -ltorch_cpu -ltorch_python" % (tlib, tlib)
    hiplibs = "%s -lc10_hip -ltorch_hip -lamdhip64 -lrccl" % tlibs

    lines = [
        "ninja_required_version = 1.3",
        "hipcc = %s" % hipcc,
        "cxx = g++",
        "rule hip",
        "  command = $hipcc %s -MD -MF $out.d -c $in -o $out" % hipflags,
        "  depfile = $out.d",
        "  deps = gcc",
        "  description = HIPCC $in",
        "rule bind",
        "  command = $cxx %s -MD -MF $out.d -c $in -o $out" % bindflags,
        "  depfile = $out.d",
        "  deps = gcc",
        "  description = CXX(bind) $in",
        "rule host",
        "  command = $cxx %s -MD -MF $out.d -c $in -o $out" % hostflags,
        "  depfile = $out.d",
        "  deps = gcc",
        "  description = CXX(host) $in",
        "rule link_hip",
        "  command = $hipcc --offload-arch=%s -shared -fPIC $in -o $out %s" % (ARCH, hiplibs),
        "  description = LINK $out",
        "rule link_host",
        "  command = $cxx -shared -fPIC -pthread $in -o $out %s -lssl -lcrypto" % tlibs,
        "  description = LINK $out",
        "rule tool",
        "  command = $cxx -O3 -std=c++17 -Wall -Wno-sign-compare -pthread -I%s/csrc -MD -MF $out.d -c $in -o $out" % ROOT,
        "  depfile = $out.d",
        "  deps = gcc",
        "  description = CXX(tool) $in",
        "rule link_tool",
        "  command = $cxx -pthread $in -o $out -lssl -lcrypto",
        "  description = LINK $out",
    ]
    hip_objs = []
    for src in sorted(glob.glob(os.path.join(ROOT, "csrc/hip/*.hip"))):
        obj = os.path.join(BUILD, "hip", os.path.basename(src) + ".o")
        lines.append("build %s: hip %s" % (obj, src))
        hip_objs.append(obj)
    for src in sorted(glob.glob(os.path.join(ROOT, "csrc/bind/*.cc"))):
        obj = os.path.join(BUILD, "bind", os.path.basename(src) + ".o")
        lines.append("build %s: bind %s" % (obj, src))
        hip_objs.append(obj)
    host_objs = []
    for src in sorted(glob.glob(os.path.join(ROOT, "csrc/host/*.cc"))):
        obj = os.path.join(BUILD, "host", os.path.basename(src) + ".o")
        lines.append("build %s: host %s" % (obj, src))
        host_objs.append(obj)
    # standalone native tools (no torch): bin/native/{convert,text2crb}
    core = []
    for name in ("parsers", "io", "remote_fs", "json", "lz4", "cityhash"):
        obj = os.path.join(BUILD, "tool", name + ".o")
        lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, "csrc/host/%s.cc" % name)))
        core.append(obj)
    lib = os.path.join(BUILD, "tool", "convert_lib.o")
    lines.append("build %s: tool %s" % (lib, os.path.join(ROOT, "csrc/tools/convert_lib.cc")))
    core.append(lib)
    for tool in ("convert", "text2crb"):
        obj = os.path.join(BUILD, "tool", tool + ".o")
        lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, "csrc/tools/%s.cc" % tool)))
        lines.append("build %s: link_tool %s %s" % (os.path.join(ROOT, "bin", "native", tool), obj,
                                                    " ".join(core)))
    # host runtime self-test (no torch): bin/native/host_selftest
    st = []
    for name in ("workload_pool", "conf_parser", "van"):
        obj = os.path.join(BUILD, "tool", name + ".o")
        lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, "csrc/host/%s.cc" % name)))
        st.append(obj)
    obj = os.path.join(BUILD, "tool", "host_selftest.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, "csrc/tests/host_selftest.cc")))
    lines.append("build %s: link_tool %s %s %s" % (
        os.path.join(ROOT, "bin", "native", "host_selftest"), obj, " ".join(st),
        " ".join(o for o in core if not o.endswith("convert_lib.o"))))
    # ranking task plan test (header only: no torch, no HIP): bin/native/gbdt_rank_plan_test
    obj = os.path.join(BUILD, "tool", "gbdt_rank_plan_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, RANK_PLAN_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_rank_plan_test"), obj))
    # contribution tables and plan test (header only): bin/native/gbdt_shap_plan_test
    obj = os.path.join(BUILD, "tool", "gbdt_shap_plan_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, SHAP_PLAN_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_shap_plan_test"), obj))
    # interaction references test (header only): bin/native/gbdt_shap_inter_test
    obj = os.path.join(BUILD, "tool", "gbdt_shap_inter_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, SHAP_INTER_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_shap_inter_test"), obj))
    # DART tree table and walk plan test (header only): bin/native/gbdt_dart_plan_test
    obj = os.path.join(BUILD, "tool", "gbdt_dart_plan_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, DART_PLAN_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_dart_plan_test"), obj))
    # quantile select plan test (header only): bin/native/gbdt_quantile_plan_test
    obj = os.path.join(BUILD, "tool", "gbdt_quantile_plan_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, QUANTILE_PLAN_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_quantile_plan_test"), obj))
    # best-first growth bookkeeping test (header only): bin/native/gbdt_leaf_plan_test
    obj = os.path.join(BUILD, "tool", "gbdt_leaf_plan_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, LEAF_PLAN_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_leaf_plan_test"), obj))
    # survival plan and AFT pair test (header only): bin/native/gbdt_survival_plan_test
    obj = os.path.join(BUILD, "tool", "gbdt_survival_plan_test.o")
    lines.append("build %s: tool %s" % (obj, os.path.join(ROOT, SURVIVAL_PLAN_TEST_SRC)))
    lines.append("build %s: link_tool %s" % (
        os.path.join(ROOT, "bin", "native", "gbdt_survival_plan_test"), obj))
    lines.append("build %s: link_hip %s" % (os.path.join(PKG, "_hip.so"), " ".join(hip_objs)))
    lines.append("build %s: link_host %s" % (os.path.join(PKG, "_host.so"), " ".join(host_objs)))
    os.makedirs(BUILD, exist_ok=True)
    with open(os.path.join(BUILD, "build.ninja"), "w") as f:
        f.write("\n".join(lines) + "\n")


RANK_PLAN_TEST_SRC = "csrc/tests/gbdt_rank_plan_test.cc"
SHAP_PLAN_TEST_SRC = "csrc/tests/gbdt_shap_plan_test.cc"
SHAP_INTER_TEST_SRC = "csrc/tests/gbdt_shap_inter_test.cc"
DART_PLAN_TEST_SRC = "csrc/tests/gbdt_dart_plan_test.cc"
QUANTILE_PLAN_TEST_SRC = "csrc/tests/gbdt_quantile_plan_test.cc"
LEAF_PLAN_TEST_SRC = "csrc/tests/gbdt_leaf_plan_test.cc"
SURVIVAL_PLAN_TEST_SRC = "csrc/tests/gbdt_survival_plan_test.cc"
SELFTEST_SRCS = ("csrc/tests/host_selftest.cc", "csrc/host/parsers.cc", "csrc/host/io.cc",
                 "csrc/host/remote_fs.cc", "csrc/host/lz4.cc", "csrc/host/cityhash.cc", "csrc/host/workload_pool.cc",
                 "csrc/host/conf_parser.cc", "csrc/host/van.cc", "csrc/host/json.cc")


def build_sanitized(kind, jobs=None):
    """The host self-test under -fsanitize=<kind> (address | thread |
    undefined), host code only: build/san-<kind>/host_selftest."""
    out_dir = os.path.join(BUILD, "san-" + kind)
    os.makedirs(out_dir, exist_ok=True)
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fno-omit-frame-pointer",
             "-fsanitize=" + kind, "-I" + os.path.join(ROOT, "csrc")]
    objs = []
    for src in SELFTEST_SRCS:
        obj = os.path.join(out_dir, os.path.basename(src) + ".o")
        subprocess.run(["g++"] + flags + ["-c", os.path.join(ROOT, src), "-o", obj], check=True)
        objs.append(obj)
    exe = os.path.join(out_dir, "host_selftest")
    subprocess.run(["g++"] + flags + objs + ["-o", exe, "-lssl", "-lcrypto"], check=True)
    return exe


def _build_plan_test_sanitized(name, src):
    """A header-only plan test (its own main) under
    -fsanitize=address,undefined: build/san-<name>/<test>."""
    out_dir = os.path.join(BUILD, "san-" + name)
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0])
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "csrc"), os.path.join(ROOT, src),
                    "-o", exe], check=True)
    return exe


def build_rank_plan_sanitized():
    """The ranking task plan test (csrc/host/gbdt_rank_plan.h, its own main)
    under -fsanitize=address,undefined: build/san-rank-plan/gbdt_rank_plan_test.
    The plain build is bin/native/gbdt_rank_plan_test."""
    return _build_plan_test_sanitized("rank-plan", RANK_PLAN_TEST_SRC)


def build_shap_plan_sanitized():
    """The contribution tables and plan test (csrc/host/gbdt_shap_plan.h, its
    own main) under -fsanitize=address,undefined:
    build/san-shap-plan/gbdt_shap_plan_test. The plain build is
    bin/native/gbdt_shap_plan_test."""
    return _build_plan_test_sanitized("shap-plan", SHAP_PLAN_TEST_SRC)


def build_shap_inter_sanitized():
    """The interaction references test (csrc/host/gbdt_shap_plan.h, its own
    main) under -fsanitize=address,undefined:
    build/san-shap-inter/gbdt_shap_inter_test. The plain build is
    bin/native/gbdt_shap_inter_test."""
    return _build_plan_test_sanitized("shap-inter", SHAP_INTER_TEST_SRC)


def build_dart_plan_sanitized():
    """The DART tree table and walk plan test (csrc/host/gbdt_dart_plan.h, its
    own main) under -fsanitize=address,undefined:
    build/san-dart-plan/gbdt_dart_plan_test. The plain build is
    bin/native/gbdt_dart_plan_test."""
    return _build_plan_test_sanitized("dart-plan", DART_PLAN_TEST_SRC)


def build_quantile_plan_sanitized():
    """The quantile select plan test (csrc/host/gbdt_quantile_plan.h, its own
    main) under -fsanitize=address,undefined:
    build/san-quantile-plan/gbdt_quantile_plan_test. The plain build is
    bin/native/gbdt_quantile_plan_test."""
    return _build_plan_test_sanitized("quantile-plan", QUANTILE_PLAN_TEST_SRC)


def build_leaf_plan_sanitized():
    """The best-first growth bookkeeping test (csrc/host/gbdt_leaf_plan.h, its
    own main) under -fsanitize=address,undefined:
    build/san-leaf-plan/gbdt_leaf_plan_test. The plain build is
    bin/native/gbdt_leaf_plan_test."""
    return _build_plan_test_sanitized("leaf-plan", LEAF_PLAN_TEST_SRC)


def build_survival_plan_sanitized():
    """The survival plan and AFT pair test (csrc/host/gbdt_survival_plan.h,
    csrc/host/gbdt_aft.h, its own main) under -fsanitize=address,undefined:
    build/san-survival-plan/gbdt_survival_plan_test. The plain build is
    bin/native/gbdt_survival_plan_test."""
    return _build_plan_test_sanitized("survival-plan", SURVIVAL_PLAN_TEST_SRC)


def build(jobs=None, clean=False, verbose=False):
    if clean and os.path.isdir(BUILD):
        shutil.rmtree(BUILD)
    gen_ninja()
    jobs = jobs or min(16, os.cpu_count() or 4)
    cmd = ["ninja", "-C", BUILD, "-j", str(jobs)]
    if verbose:
        cmd.append("-v")
    r = subprocess.run(cmd)
    if r.returncode != 0:
        raise SystemExit("native build failed (exit %d)" % r.returncode)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=None)
    ap.add_argument("--clean", action="store_true")
    ap.add_argument("-v", action="store_true")
    ap.add_argument("--sanitize", choices=["address", "thread", "undefined"], default=None,
                    help="build the host self-test under a sanitizer instead")
    ap.add_argument("--sanitize-rank-plan", action="store_true",
                    help="build the ranking task plan test under address,undefined instead")
    ap.add_argument("--sanitize-shap-plan", action="store_true",
                    help="build the contribution plan test under address,undefined instead")
    ap.add_argument("--sanitize-shap-inter", action="store_true",
                    help="build the interaction references test under address,undefined instead")
    ap.add_argument("--sanitize-dart-plan", action="store_true",
                    help="build the DART plan test under address,undefined instead")
    ap.add_argument("--sanitize-quantile-plan", action="store_true",
                    help="build the quantile select plan test under address,undefined instead")
    ap.add_argument("--sanitize-leaf-plan", action="store_true",
                    help="build the best-first growth plan test under address,undefined instead")
    ap.add_argument("--sanitize-survival-plan", action="store_true",
                    help="build the survival plan test under address,undefined instead")
    a = ap.parse_args()
    if a.sanitize_survival_plan:
        print(build_survival_plan_sanitized())
        sys.exit(0)
    if a.sanitize_leaf_plan:
        print(build_leaf_plan_sanitized())
        sys.exit(0)
    if a.sanitize_quantile_plan:
        print(build_quantile_plan_sanitized())
        sys.exit(0)
    if a.sanitize_dart_plan:
        print(build_dart_plan_sanitized())
        sys.exit(0)
    if a.sanitize_shap_inter:
        print(build_shap_inter_sanitized())
        sys.exit(0)
    if a.sanitize_shap_plan:
        print(build_shap_plan_sanitized())
        sys.exit(0)
    if a.sanitize_rank_plan:
        print(build_rank_plan_sanitized())
        sys.exit(0)
    if a.sanitize:
        print(build_sanitized(a.sanitize, a.j))
        sys.exit(0)
    build(a.j, a.clean, a.v)
    sys.exit(0)
