"""Are the kernels of one source file still the kernels they were?  Compiles the device side of a .hip file of two
trees to gfx950 assembly (no GPU needed) and compares every function the two have in common, instruction for
instruction:

    python tools/compare_kernel_asm.py OLD_TREE NEW_TREE hybridbackend_amd/csrc/hash_insert.hip

Prints the count of functions compared, the names that only one side has, and every function whose code differs;
exits 1 when a common function differs.  Labels, comments and assembler directives are not code: a function that
moved in the file compares equal.  Symbols are printed demangled where c++filt is at hand."""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fno-fast-math', '-ffp-contract=off', '--cuda-device-only',
         '-S']


def device_asm(tree, source):
  rocm = os.environ.get('ROCM', '/opt/rocm')
  with tempfile.TemporaryDirectory() as tmp:
    out = os.path.join(tmp, 'device.s')
    subprocess.check_call([os.path.join(rocm, 'bin', 'hipcc')] + FLAGS + [
      '-I' + os.path.join(tree, 'include'), '-I' + os.path.join(rocm, 'include'), os.path.join(tree, source), '-o', out])
    return open(out).read()


def functions(asm):
  """name -> list of instruction lines, local labels renumbered in order of appearance."""
  out = {}
  for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:', asm, flags=re.S | re.M):
    labels, code = {}, []
    for line in m.group(2).split('\n'):
      line = line.split(';')[0].strip()
      if not line or line.startswith('.') and not line.startswith('.LBB'):
        continue
      code.append(line)
    for line in code:
      if line.endswith(':'):
        labels.setdefault(line[:-1], f'L{len(labels)}')
    rename = lambda t: re.sub(r'\.LBB\d+_\d+', lambda k: labels.get(k.group(0), k.group(0)), t)   # noqa: E731
    out[m.group(1)] = [rename(line) for line in code]
  return out


def demangle(names):
  try:
    got = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, got.split('\n')))
  except (OSError, subprocess.CalledProcessError):
    return {n: n for n in names}


def main(argv):
  if len(argv) != 4:
    sys.exit(__doc__)
  old, new = (functions(device_asm(tree, argv[3])) for tree in argv[1:3])
  both = sorted(set(old) & set(new))
  pretty = demangle(sorted(set(old) | set(new)))
  differ = [n for n in both if old[n] != new[n]]
  print(f'{argv[3]}: {len(both)} functions compared, {len(both) - len(differ)} identical, {len(differ)} differ')
  for n in both:
    print(f'  {"DIFFERS" if n in differ else "same   "} {len(new[n]):6d} lines  {pretty[n]}')
  for side, only in (('old', set(old) - set(new)), ('new', set(new) - set(old))):
    for n in sorted(only):
      print(f'  only in the {side} tree: {pretty[n]}')
  return 1 if differ else 0


if __name__ == '__main__':
  sys.exit(main(sys.argv))
