"""Emit the launch planner's rate table from a measurement pass's bench lines.

Usage: python tools/make_rates.py OUT.txt DIR [DIR ...]

Reads the bench JSON lines of the probes tools/measure_r06.sh writes (each at a forced rows per
group, WRNN_PERSIST_NR_MAX=k and no rotation / slicing, so `us_per_step` is that variant's step
time) and writes `key v1 .. v4` lines for the keys it found; the runtime
(plan.cpp load_rates) overrides those keys of its built-in defaults and keeps the rest:
  <dir>/nr<k>.log      -> fat9      (fatchord 9-bit, C2 shape)
  <dir>/u10_nr<k>.log  -> fat10     (fatchord 10-bit, its 3000 / 1500 default)
  <dir>/sp_nr<k>.log   -> fat9_sp   (sparse instances, 90 %-pruned weights)
  <dir>/rr_nr<k>.log   -> rr        <dir>/gen_nr<k>.log -> gen
  <dir>/c4.log (16 rows / group, 512 classes), <dir>/b10.log (16 rows, 1024 classes),
  <dir>/u10_wide.log (6 rows, 1024 classes) -> wide = base, per row, 1024-class extra
  <dir>/mol_wide_r<k>.log (fatchord MOL, every launch wide at k rows per group, WRNN_PERSIST_WIDE=1;
    at least two fills, e.g. k = 5 and 16) -> wide_mol = base, per row (least squares)
  <dir>/gen_wide_r<k>.log (geneing BITS, every launch wide at k rows per group, WRNN_PERSIST_WIDE=1;
    at least two fills) -> wide_gen = base, per row (least squares)
  <dir>/rr_mol_wide_r<k>.log (runtimeracer MOL, every launch wide at k rows per group,
    WRNN_PERSIST_WIDE=1; at least two fills) -> wide_rr_mol = base, per row (least squares)
  <dir>/gen_mol_wide_r<k>.log, <dir>/gen_beta_wide_r<k>.log (geneing MOL / Beta ('RAW'), every launch
    wide at k rows per group, WRNN_PERSIST_WIDE=1; at least two fills) -> wide_gen_mol,
    wide_gen_beta = base, per row (least squares)
  <dir>/gen32_wide_r<k>.log, <dir>/gen32_mol_wide_r<k>.log, <dir>/gen32_beta_wide_r<k>.log (geneing BITS /
    MOL / Beta, one 32-row launch at k = 17 .. 32 rows per group, WRNN_PERSIST_WIDE=1 and
    WRNN_GEN_WIDE_ROWS=32; at least two fills) -> wide_gen32, wide_gen32_mol, wide_gen32_beta = base,
    per row (least squares)
  <dir>/gen_slice_r16.log, <dir>/gen_slice_mol_r16.log, <dir>/gen_slice_beta_r16.log (geneing BITS / MOL /
    Beta, a time-sliced call, WRNN_GEN_SLICE=1: `us_per_step` is the mean step of its launches, which
    run 16 rows per group but for the short tails) -> wide_gen_slice, wide_gen_slice_mol,
    wide_gen_slice_beta = base, per row: one fill, so the per-row term is that of the head's unsliced
    key (wide_gen, wide_gen_mol, wide_gen_beta), from this pass or else from the table given as OUT
  <dir>/sp_wide_r<k>.log, <dir>/sp10_wide_r<k>.log (fatchord RAW at 9 / 10 bits on 90 %-pruned weights,
    every launch block-sparse wide at k rows per group, WRNN_PERSIST_WIDE=1 and WRNN_SPARSE_WIDE=1), or
    <dir>/rates.log (stage-timing lines {"bits", "rows_per_group", "kernel", "us_per_step"}; the
    `persist_wide_sp` lines, repeats of a point averaged: profiles/wide_sp); at least two 9-bit
    fills and one 10-bit fill -> wide_sp = base, per row (least squares over the 9-bit fills),
    1024-class extra (mean excess of the 10-bit fills over that line)
Later directories override earlier ones. The rotation tables keep the runtime's defaults unless
a key is already in the file given as OUT (kept lines are carried over).
"""
import json
import os
import sys

FAMILIES = {'nr': 'fat9', 'u10_nr': 'fat10', 'sp_nr': 'fat9_sp', 'rr_nr': 'rr', 'gen_nr': 'gen'}


def table_of(path):
    """{key: [values]} of the key lines of a rate table (none when there is no such file)."""
    tab = {}
    try:
        for ln in open(path):
            k = ln.split('#')[0].split()
            if k:
                tab[k[0]] = [float(v) for v in k[1:]]
    except OSError:
        pass
    return tab


def line_of(path):
    try:
        for ln in open(path):
            if ln.startswith('{'):
                return json.loads(ln)
    except OSError:
        return None
    return None


def us_step(d):
    r = (d or {}).get('roofline') or {}
    return r.get('us_per_step')


def main():
    out, dirs = sys.argv[1], sys.argv[2:]
    keys, src = {}, {}
    for d in dirs:
        for pre, key in FAMILIES.items():
            vals = [us_step(line_of(os.path.join(d, f'{pre}{k}.log'))) for k in (1, 2, 3, 4)]
            if all(v is not None for v in vals):
                keys[key] = [round(v, 3) for v in vals]
                src[key] = d
        c4, b10, u10w = (us_step(line_of(os.path.join(d, f))) for f in ('c4.log', 'b10.log', 'u10_wide.log'))
        if c4 and b10:
            extra = b10 - c4
            per_row = ((b10 - extra) - (u10w - extra)) / 10.0 if u10w else 0.025
            per_row = max(per_row, 0.001)
            keys['wide'] = [round(c4 - 16 * per_row, 3), round(per_row, 4), round(extra, 3)]
            src['wide'] = d
        pts = [(k, us_step(line_of(os.path.join(d, f'mol_wide_r{k}.log')))) for k in range(1, 17)]
        pts = [(k, v) for k, v in pts if v is not None]
        if len(pts) >= 2:
            mk, mv = sum(k for k, _ in pts) / len(pts), sum(v for _, v in pts) / len(pts)
            per_row = sum((k - mk) * (v - mv) for k, v in pts) / sum((k - mk) ** 2 for k, _ in pts)
            per_row = max(per_row, 0.001)
            keys['wide_mol'] = [round(mv - per_row * mk, 3), round(per_row, 4)]
            src['wide_mol'] = d
        pts = [(k, us_step(line_of(os.path.join(d, f'gen_wide_r{k}.log')))) for k in range(1, 17)]
        pts = [(k, v) for k, v in pts if v is not None]
        if len(pts) >= 2:
            mk, mv = sum(k for k, _ in pts) / len(pts), sum(v for _, v in pts) / len(pts)
            per_row = sum((k - mk) * (v - mv) for k, v in pts) / sum((k - mk) ** 2 for k, _ in pts)
            per_row = max(per_row, 0.001)
            keys['wide_gen'] = [round(mv - per_row * mk, 3), round(per_row, 4)]
            src['wide_gen'] = d
        pts = [(k, us_step(line_of(os.path.join(d, f'rr_mol_wide_r{k}.log')))) for k in range(1, 17)]
        pts = [(k, v) for k, v in pts if v is not None]
        if len(pts) >= 2:
            mk, mv = sum(k for k, _ in pts) / len(pts), sum(v for _, v in pts) / len(pts)
            per_row = sum((k - mk) * (v - mv) for k, v in pts) / sum((k - mk) ** 2 for k, _ in pts)
            per_row = max(per_row, 0.001)
            keys['wide_rr_mol'] = [round(mv - per_row * mk, 3), round(per_row, 4)]
            src['wide_rr_mol'] = d
        for pre, key in (('gen_mol_wide_r', 'wide_gen_mol'), ('gen_beta_wide_r', 'wide_gen_beta')):
            pts = [(k, us_step(line_of(os.path.join(d, f'{pre}{k}.log')))) for k in range(1, 17)]
            pts = [(k, v) for k, v in pts if v is not None]
            if len(pts) >= 2:
                mk, mv = sum(k for k, _ in pts) / len(pts), sum(v for _, v in pts) / len(pts)
                per_row = sum((k - mk) * (v - mv) for k, v in pts) / sum((k - mk) ** 2 for k, _ in pts)
                per_row = max(per_row, 0.001)
                keys[key] = [round(mv - per_row * mk, 3), round(per_row, 4)]
                src[key] = d
        for pre, key in (('gen32_wide_r', 'wide_gen32'), ('gen32_mol_wide_r', 'wide_gen32_mol'),
                         ('gen32_beta_wide_r', 'wide_gen32_beta')):
            pts = [(k, us_step(line_of(os.path.join(d, f'{pre}{k}.log')))) for k in range(17, 33)]
            pts = [(k, v) for k, v in pts if v is not None]
            if len(pts) >= 2:
                mk, mv = sum(k for k, _ in pts) / len(pts), sum(v for _, v in pts) / len(pts)
                per_row = sum((k - mk) * (v - mv) for k, v in pts) / sum((k - mk) ** 2 for k, _ in pts)
                per_row = max(per_row, 0.001)
                keys[key] = [round(mv - per_row * mk, 3), round(per_row, 4)]
                src[key] = d
        for pre, key, head in (('gen_slice_r', 'wide_gen_slice', 'wide_gen'),
                               ('gen_slice_mol_r', 'wide_gen_slice_mol', 'wide_gen_mol'),
                               ('gen_slice_beta_r', 'wide_gen_slice_beta', 'wide_gen_beta')):
            # one fill: every sliced launch but the short tails runs 16 rows per group. The per-row
            # term is the head's unsliced key's, of this pass or else of the table given as OUT
            v16 = us_step(line_of(os.path.join(d, f'{pre}16.log')))
            if v16 is None:
                continue
            unsliced = keys.get(head) or table_of(out).get(head)
            if not unsliced or len(unsliced) != 2:
                print(f'{key}: skipped, no {head} key in this pass or in {out}', file=sys.stderr)
                continue
            keys[key] = [round(v16 - unsliced[1] * 16, 3), unsliced[1]]
            src[key] = d
        pts = [(k, us_step(line_of(os.path.join(d, f'sp_wide_r{k}.log')))) for k in range(1, 17)]
        pts = [(k, v) for k, v in pts if v is not None]
        pts10 = [(k, us_step(line_of(os.path.join(d, f'sp10_wide_r{k}.log')))) for k in range(1, 17)]
        pts10 = [(k, v) for k, v in pts10 if v is not None]
        try:
            pt = {}
            for ln in open(os.path.join(d, 'rates.log')):
                j = json.loads(ln) if ln.startswith('{') else {}
                if j.get('kernel') == 'persist_wide_sp':
                    pt.setdefault((j['bits'], j['rows_per_group']), []).append(j['us_per_step'])
            pts += [(k, sum(v) / len(v)) for (b, k), v in sorted(pt.items()) if b == 9]
            pts10 += [(k, sum(v) / len(v)) for (b, k), v in sorted(pt.items()) if b == 10]
        except OSError:
            pass
        if len(pts) >= 2 and pts10:
            mk, mv = sum(k for k, _ in pts) / len(pts), sum(v for _, v in pts) / len(pts)
            per_row = sum((k - mk) * (v - mv) for k, v in pts) / sum((k - mk) ** 2 for k, _ in pts)
            per_row = max(per_row, 0.001)
            base = mv - per_row * mk
            extra = max(sum(v - (base + per_row * k) for k, v in pts10) / len(pts10), 0.001)
            keys['wide_sp'] = [round(base, 3), round(per_row, 4), round(extra, 3)]
            src['wide_sp'] = d
    kept = []
    if os.path.exists(out):
        for ln in open(out):
            k = ln.split('#')[0].split()
            if k and k[0] not in keys:
                kept.append(ln.rstrip('\n'))
    with open(out, 'w') as f:
        f.write('# MI355X launch-planner rates (us per step), written by tools/make_rates.py from\n')
        for k in sorted(keys):
            f.write(f'#   {k}: {src[k]}\n')
        for k in sorted(keys):
            f.write(k + ' ' + ' '.join(str(v) for v in keys[k]) + '\n')
        for ln in kept:
            if not ln.startswith('#'):
                f.write(ln + '\n')
    print(open(out).read())


if __name__ == '__main__':
    main()
