"""What the host checks (test_host_plan.py, test_host_motion.py, test_host_loss.py) share: the compiler search, the sanitized build line
of a stand-alone checker under tests/host/, and the case file that one run of it, as a child process, answers.  Nothing is preloaded."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'edge-informed-contrast-maximization_amd', 'csrc')
SANITIZE = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def compiler():
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cxx in ('g++', os.path.join(rocm, 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++')):
        if shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError('neither g++ nor the ROCm clang++ found')


def build(tmp_path_factory, name, extra=()):
    """Path of the sanitized checker built from tests/host/<name>.cpp."""
    exe = str(tmp_path_factory.mktemp(name) / name)
    cxx = compiler()
    # (g++ links the sanitizers' runtimes into the program, as clang++ does by default: the program needs nothing preloaded)
    static = ['-static-libasan', '-static-libubsan'] if os.path.basename(cxx) == 'g++' else []
    cmd = [cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SANITIZE + list(extra) + static + [
        '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'host', name + '.cpp')]
    print(' '.join(cmd))
    assert '-fsanitize=address,undefined' in cmd and '-fno-sanitize-recover=all' in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def token(t):
    if isinstance(t, (bool, int, np.integer)):
        return str(int(t))
    return repr(float(t)) if isinstance(t, (float, np.floating)) else str(t)


def add_case(cases, name, *tokens):
    """cases[name] = the input line: the checker's case word, then integers and floats (repr: they read back to the same doubles)."""
    assert name not in cases, name
    cases[name] = ' '.join(token(t) for t in tokens)
    return name


def run(exe, cases, tmp_path_factory, tag):
    """name -> the checker's line for that case, split at ' |' into lists of words."""
    path = tmp_path_factory.mktemp(tag) / 'cases.txt'
    path.write_text('\n'.join(cases.values()) + '\n')
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f'the sanitized checker failed (exit {r.returncode}):\n{r.stderr[-4000:]}'
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    res = {}
    for (name, inp), line in zip(cases.items(), lines):
        word, _, rest = line.partition(' ')
        assert word == inp.split()[0]
        res[name] = [part.split() for part in rest.split('|')]
    return res


def f(tokens):
    return np.array([float(t) for t in tokens], dtype=np.float64)


def i(tokens):
    return np.array([int(t) for t in tokens], dtype=np.int64)
