"""Instruction statistics from hipcc -S --offload-device-only assembly files.

One kernel, its instruction mix:
   python3 tools/isa_stats.py /tmp/txh_prefilter.s adc_smfmac_kernelILi32 [--dump out.s]
Every kernel of one or more files, one line each (sorted by name), to compare two builds of the same kernels:
   python3 tools/isa_stats.py --table /tmp/txh.s /tmp/txh_prefilter.s ... > table.tsv
The files come from `hipcc <build.py CFLAGS> --offload-device-only -S -o unit.s unit.hip`."""
import collections
import hashlib
import re
import sys

META = ["vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size"]


def one_kernel(path, name, dump=None):
    s = open(path).read()
    m = re.search(r'^(_ZN\S*%s\S*):' % re.escape(name), s, re.M)
    i = m.start()
    j = s.index('.end_amdhsa_kernel', i)
    body = s[i:j]
    lines = body.split('\n')
    cnt = collections.Counter()
    for l in lines:
        mm = re.match(r'\s+([a-z_0-9]+)', l)
        if mm:
            cnt[mm.group(1)] += 1
    print(m.group(1), len(lines), 'lines')
    print('mfma', sum(v for k, v in cnt.items() if 'mfma' in k), 'scratch', sum(v for k, v in cnt.items() if k.startswith('scratch_')))
    print(cnt.most_common(45))
    if dump:
        open(dump, 'w').write(body)


def kernel_metadata(s):
    """{mangled name: {field: value}} from the amdhsa.kernels list of the file's metadata note."""
    out = {}
    i = s.index('\namdhsa.kernels:')
    cur = None
    for l in s[i:].split('\n')[2:]:
        if not l.startswith('  '):
            break
        m = re.match(r'^(  - |    )\.(\w+):\s*(\S*)', l)   # keys of a kernel's own map (its .args are nested deeper)
        if not m:
            continue
        if m.group(1) == '  - ':
            cur = {}
        cur[m.group(2)] = m.group(3)
        if m.group(2) == 'name':
            out[m.group(3)] = cur
    return out


def instruction_stream(s, name):
    """(instruction lines, sha256 of the stream) of one kernel: comments dropped, .LBB<n>_<m> labels renumbered by
    first appearance, so that the position of the kernel in its file does not show."""
    i = s.index('\n%s:' % name) + 1
    j = re.compile(r'^\.Lfunc_end\d+:', re.M).search(s, i).start()
    labels = {}
    relabel = lambda m: labels.setdefault(m.group(0), '.LBB_%d' % len(labels))
    n, h = 0, hashlib.sha256()
    for l in s[i:j].split('\n')[1:]:
        l = l.split(';')[0].strip()
        if not l:
            continue
        l = re.sub(r'\s+', ' ', re.sub(r'\.LBB\d+_\d+', relabel, l))
        if re.match(r'[a-z]', l):
            n += 1
        h.update(l.encode() + b'\n')
    return n, h.hexdigest()[:16]


def table(paths):
    rows, seen = [], collections.Counter()
    for p in paths:
        s = open(p).read()
        for name, md in kernel_metadata(s).items():
            seen[name] += 1
            n, digest = instruction_stream(s, name)
            rows.append([name] + [md.get(f, '?') for f in META] + [str(n), digest])
    print('\t'.join(['kernel'] + META + ['instructions', 'stream_sha256']))
    for r in sorted(rows):
        print('\t'.join(r))
    twice = [k for k, v in seen.items() if v > 1]
    print('# %d kernels%s' % (len(seen), ', MORE THAN ONCE: ' + ' '.join(twice) if twice else ''))
    return 1 if twice else 0


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--table':
        sys.exit(table(sys.argv[2:]))
    one_kernel(sys.argv[1], sys.argv[2], sys.argv[sys.argv.index('--dump') + 1] if '--dump' in sys.argv else None)
