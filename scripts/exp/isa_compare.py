"""Compare the gfx950 device code of some units between two source trees, kernel by kernel, without a GPU.

  python scripts/exp/isa_compare.py PARENT_TREE NEW_TREE loss.hip semi.hip score.hip elementwise.hip

Each unit is compiled to assembly with the flags of lidal_amd/build.py (of the tree it comes from).  A kernel's
instructions are its lines between the label and .Lfunc_end, comments, labels of basic blocks and debug directives
dropped.  Prints, for every kernel whose instructions differ (or that exists in one tree only): VGPRs, SGPRs, scratch
bytes, LDS bytes and waves per SIMD, parent -> new, as a markdown table; and the number of identical kernels.
"""
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile


def flags_of(tree):
    spec = importlib.util.spec_from_file_location('b', os.path.join(tree, 'lidal_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return lambda unit: b.FLAGS + b.NO_PACKED_F32 + (['-ffp-contract=off'] if unit in b.NO_CONTRACT else [])


def kernels_of(tree, unit, tmp):
    out = os.path.join(tmp, unit + '.s')
    cmd = ['hipcc'] + flags_of(tree)(unit) + ['--cuda-device-only', '-S', os.path.join(tree, 'lidal_amd', 'csrc', unit),
                                             '-o', out]
    subprocess.run(cmd, check=True)
    text = open(out).read()
    res = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = re.search(r'\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel' % re.escape(name), text, re.S)
        if meta is None:
            continue                                  # a device function, not a kernel
        # (a branch target carries the function's number in the unit, which moves when a kernel becomes a template)
        ins = [re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].strip()) for ln in body.split('\n')]
        ins = [ln for ln in ins if ln and not ln.startswith('.') and not ln.endswith(':')]
        tail = text[m.end():m.end() + 4000]
        get = lambda key: int(re.search(r'; %s: (\d+)' % key, tail).group(1))
        res[name] = dict(ins=ins, vgpr=get('TotalNumVgprs'), sgpr=get('TotalNumSgprs'), scratch=get('ScratchSize'),
                         lds=get('LDSByteSize'), waves=get('Occupancy'))
    return res


def demangle(name):
    rocm = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'llvm-cxxfilt')      # knows __bf16
    tool = rocm if os.path.exists(rocm) else shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not tool:
        return name
    full = subprocess.run([tool, name], capture_output=True, text=True).stdout.strip()
    full = re.sub(r'^void ', '', full.replace('(anonymous namespace)::', '').replace('lidal::', ''))
    depth = 0
    for at, ch in enumerate(full):                    # cut the argument list, keep the template arguments
        depth += ch == '<'
        depth -= ch == '>'
        if ch == '(' and depth == 0:
            return full[:at]
    return full


def main():
    parent, new, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    same = 0
    print('| kernel | instructions | VGPRs | SGPRs | scratch B | LDS B | waves/SIMD |\n|---|---|---|---|---|---|---|')
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for unit in units:
            a, b = kernels_of(parent, unit, ta), kernels_of(new, unit, tb)
            for name in sorted(set(a) | set(b)):
                ka, kb = a.get(name), b.get(name)
                if ka and kb and ka['ins'] == kb['ins']:
                    same += 1
                    continue
                col = lambda key: '%s -> %s' % (ka[key] if ka else '-', kb[key] if kb else '-')
                nins = '%s -> %s' % (len(ka['ins']) if ka else '-', len(kb['ins']) if kb else '-')
                print('| `%s` (%s) | %s | %s | %s | %s | %s | %s |' % (demangle(name), unit, nins, col('vgpr'),
                                                                    col('sgpr'), col('scratch'), col('lds'), col('waves')))
    print('\nidentical kernels: %d' % same)


if __name__ == '__main__':
    main()
