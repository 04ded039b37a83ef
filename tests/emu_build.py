"""A kernel's source as a stand-alone CPU program: the fixture body of the test_*_host.py files that run figdraw_amd/csrc/k_*.hip under a
host shim of tests/emu ("The host shims")."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")  # a program's flags for AddressSanitizer and UBSan


def build(where, driver, csrc, programs, opt="-O1", flags=(), threads=False, source="emu.cpp"):
    """where: a directory, or pytest's tmp_path_factory (a directory named after the driver is made); driver: the directory under tests/
    whose `source` is the program's main; csrc: the library's files to copy beside it, unmodified; programs: {name: the flags it adds}.
    threads: the threaded shim and the stand-in fdh_damage.h, C++20 and -lpthread; without it the sequential shim, C++17 and -w.
    -> the directory of the programs"""
    tmp = where.mktemp(driver) if hasattr(where, "mktemp") else where
    emu = os.path.join(ROOT, "tests", "emu")
    shutil.copy(os.path.join(emu, "fdh_device_threads.h" if threads else "fdh_device.h"), os.path.join(tmp, "fdh_device.h"))
    if threads:
        shutil.copy(os.path.join(emu, "fdh_damage.h"), tmp)
    shutil.copy(os.path.join(ROOT, "tests", driver, source), tmp)
    for name in csrc:
        shutil.copy(os.path.join(ROOT, "figdraw_amd", "csrc", name), tmp)
    gxx = ["g++", "-std=c++20" if threads else "-std=c++17", opt, *(() if threads else ("-w",)), *flags, "-x", "c++", source]
    for name, more in programs.items():
        subprocess.check_call(gxx + list(more) + ["-o", name] + (["-lpthread"] if threads else []), cwd=tmp)
    return tmp
