"""Every launch plan of a built library as text, one canonical line per case: the record a change
to the launch planner (csrc/plan.cpp) is compared against. Host only, through the
handle-free entry points wrnn_debug_plan / wrnn_debug_stream_bytes / wrnn_debug_rot_plan /
wrnn_debug_slice_plan; two libraries that plan alike give byte-identical dumps.

  plan   the ten heads x rows 1..72, 131, 144, 152, 232, 360, 2115, 4096 x six seq_len x every
         subset of the wrnn_debug_plan flags the head's topology reads (and all nine bits): the plan
         under the built-in rates, then p1 bytes / noise bytes / persist_ok of its streams
  rate   on a reduced row set: the plan with one rate key's shipped values x 0.25 and x 4
  rot    wrnn_debug_rot_plan, rows 9..32 at the shipped rot9 rates (maps as a digest)
  slice  wrnn_debug_slice_plan, rows 136..512 in steps of 8 (maps as a digest)
  bad    the error text of malformed tables
  rates  wrnn_get_rates of a new handle (needs a device: wrnn_create opens one; else the error)

usage: [WRNN_LIB=other.so] python tools/plan_dump.py [--only SECTION[,SECTION]] > dump.txt
"""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'real-time-voice-cloning_amd'))

FAT, RR, GEN = 0, 1, 2
RAW, MOL, BETA = 0, 1, 2
HEADS = [('fat_raw9', FAT, 9, RAW), ('fat_raw10', FAT, 10, RAW), ('fat_mol', FAT, 9, MOL),
         ('rr_raw9', RR, 9, RAW), ('rr_raw10', RR, 10, RAW), ('rr_mol', RR, 9, MOL),
         ('gen_raw9', GEN, 9, RAW), ('gen_raw10', GEN, 10, RAW), ('gen_mol', GEN, 9, MOL),
         ('gen_beta', GEN, 9, BETA)]
# (1024, the geneing time-sliced instances, came after the other nine: its flag sets are further
# lines, and every line of a set without it stays what it was)
TOPO_BITS = {FAT: (1, 2, 4, 8), RR: (2, 4, 16), GEN: (4, 32, 64, 128, 256, 1024)}
ALL_BITS = 511
ROWS = list(range(1, 73)) + [131, 144, 152, 232, 360, 2115, 4096]
ROWS_RATE = [8, 18, 33, 45, 144, 232, 360]
SEQ = [63, 64, 1200, 6000, 12100, 14000]
# the shipped table (PlanRates in csrc/plan.h), for the scaled tables of the `rate` section
SHIPPED = {
    'fat9': [4.8, 5.15, 5.91, 6.92], 'fat10': [4.21, 5.19, 6.50, 9.41],
    'fat9_sp': [4.99, 6.95, 7.99, 9.26], 'fat10_sp': [5.3, 7.3, 8.6, 11.7],
    'rr': [6.7, 7.75, 8.81, 9.87], 'gen': [2.61, 3.26, 3.91, 4.56],
    'wide': [9.32, 0.025, 1.24], 'wide_mol': [9.366, 0.0185], 'wide_rr': [12.0, 0.025],
    'wide_rr_mol': [9.285, 0.0321], 'wide_gen': [3.508, 0.0082], 'wide_gen_mol': [3.025, 0.0094],
    'wide_gen_beta': [4.84, 0.033], 'wide_gen32': [6.347, 0.0066], 'wide_gen32_mol': [3.992, 0.0222],
    'wide_gen32_beta': [6.001, 0.0835], 'slice': [60.0, 0.98],
    'wide_gen_slice': [3.46, 0.0082], 'wide_gen_slice_mol': [2.797, 0.0094], 'wide_gen_slice_beta': [4.728, 0.033],
    'rot9': [4.8, 5.22, 5.91, 6.92], 'rot9_sp': [4.99, 6.95, 7.99, 9.26], 'rot_mol3_lo': [4.70],
    'rot_rr9': [6.3, 7.0, 7.78, 8.8], 'rot_rr10': [6.5, 7.26, 8.14, 9.23],
    'rot_rrm': [5.9, 6.6, 7.42, 8.4], 'rot_gen': [1.98, 2.47, 3.12, 3.64],
    'rot_genm': [1.72, 2.15, 2.60, 3.03], 'rot': [40.0, 0.98],
}
BAD_TABLES = ['nosuchkey 1 2', 'fat9 1 2 3', 'fat9 1 2 3 x', 'wide 1 -2 3']  # tests/test_plan_rates.py


def flag_sets(model):
    bits = TOPO_BITS[model]
    sets = [sum(c) for k in range(len(bits) + 1) for c in itertools.combinations(bits, k)]
    return sorted(sets) + [ALL_BITS]


class Dump:
    def __init__(self, out):
        from wavernn_amd import _abi
        self.abi = _abi
        self.lib = _abi.load_library()
        self.out = out
        self.cap = 4096 // 8 + 8
        self.nr = (ctypes.c_int * self.cap)()
        self.wd = (ctypes.c_int * self.cap)()

    def err(self):
        return self.lib.wrnn_last_error().decode('utf-8', 'replace')

    def plan_text(self, table, model, bits, mode, rows, S, flags):
        n, rot = ctypes.c_int(), ctypes.c_int()
        rc = self.lib.wrnn_debug_plan(table.encode() if table else None, model, bits, mode, rows, S, flags,
                                      ctypes.byref(n), self.nr, self.wd, self.cap, ctypes.byref(rot))
        if rc:
            return f'rc={rc} {self.err()}'
        # runs of equal launches as count x rows-per-group and w (wide) or r (register-resident)
        runs = []
        for key, grp in itertools.groupby((self.nr[i], self.wd[i]) for i in range(min(n.value, self.cap))):
            runs.append(f'{len(list(grp))}x{key[0]}{"w" if key[1] else "r"}')
        return f'n={n.value} rot={rot.value} [{" ".join(runs)}]'

    def stream_text(self, model, bits, mode, rows, S, flags):
        p1, nz, ok = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        rc = self.lib.wrnn_debug_stream_bytes(model, bits, mode, rows, S, flags, ctypes.byref(p1),
                                              ctypes.byref(nz), ctypes.byref(ok))
        if rc:
            return f'rc={rc} {self.err()}'
        return f'p1={p1.value!r} noise={nz.value!r} ok={ok.value}'

    def plan(self):
        for name, model, bits, mode in HEADS:
            for flags in flag_sets(model):
                for rows in ROWS:
                    for S in SEQ:
                        print(f'plan {name} flags={flags} rows={rows} S={S}: '
                              f'{self.plan_text(None, model, bits, mode, rows, S, flags)} | '
                              f'{self.stream_text(model, bits, mode, rows, S, flags)}', file=self.out)

    def rate(self):
        for key, vals in SHIPPED.items():
            for scale in (0.25, 4.0):
                table = key + ' ' + ' '.join(repr(v * scale) for v in vals)
                for name, model, bits, mode in HEADS:
                    every = sum(TOPO_BITS[model])
                    for flags in (every & ~1024, ALL_BITS) + ((every,) if every & 1024 else ()):
                        for rows in ROWS_RATE:
                            for S in SEQ:
                                print(f'rate {key}x{scale} {name} flags={flags} rows={rows} S={S}: '
                                      f'{self.plan_text(table, model, bits, mode, rows, S, flags)}', file=self.out)

    def rot(self):
        us = dict(enumerate(SHIPPED['rot9'], 1))
        for rows in range(9, 33):
            q = rows // 8
            t_hi, t_lo = us.get(q + 1, us[4]), us.get(q, us[4])
            cap = 24 * 8 * (q + 1) * 2
            vm = (ctypes.c_int * cap)()
            for S in SEQ:
                k, nh, nl = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                rc = self.lib.wrnn_debug_rot_plan(rows, S, t_hi, t_lo, ctypes.byref(k), ctypes.byref(nh),
                                                  ctypes.byref(nl), vm, cap)
                maps = hashlib.sha256(bytes(vm)[:k.value * 8 * (q + 1) * 2 * 4]).hexdigest()[:16]
                print(f'rot rows={rows} S={S}: rc={rc} K={k.value} n_hi={nh.value} n_lo={nl.value} maps={maps}'
                      + (f' {self.err()}' if rc else ''), file=self.out)

    def slice(self):
        kmax = 64 + 4
        rs = (ctypes.c_int * (2 * kmax))()
        cap = kmax * 8 * 16 * 2
        vm = (ctypes.c_int * cap)()
        for rows in range(136, 513, 8):
            for S in SEQ:
                k = ctypes.c_int()
                rc = self.lib.wrnn_debug_slice_plan(rows, S, ctypes.byref(k), rs, 2 * kmax, vm, cap)
                K = k.value
                maps = hashlib.sha256(bytes(vm)[:K * 8 * 16 * 2 * 4]).hexdigest()[:16]
                launches = ' '.join(f'{rs[2 * i]}x{rs[2 * i + 1]}' for i in range(K))
                print(f'slice rows={rows} S={S}: rc={rc} K={K} [{launches}] maps={maps}'
                      + (f' {self.err()}' if rc else ''), file=self.out)

    def bad(self):
        for t in BAD_TABLES:
            print(f'bad {t!r}: {self.plan_text(t, FAT, 9, RAW, 18, 12100, 6)}', file=self.out)

    def rates(self):
        cfg = self.abi.WrnnConfig()
        for k, v in dict(model_type=FAT, mode=RAW, bits=9, rnn_dims=512, fc_dims=512, feat_dims=80, pad=2,
                         compute_dims=128, res_out_dims=128, res_blocks=10, hop_length=200, n_upsample=3).items():
            setattr(cfg, k, v)
        for i, f in enumerate((5, 5, 8)):
            cfg.upsample_factors[i] = f
        h = ctypes.c_void_p()
        rc = self.lib.wrnn_create(ctypes.byref(cfg), 0, ctypes.byref(h))
        if rc:
            print(f'rates: no handle (rc={rc} {self.err()})', file=self.out)
            return
        buf = ctypes.create_string_buffer(4096)
        rc = self.lib.wrnn_get_rates(h, buf, 4096)
        for line in buf.value.decode().splitlines():
            print(f'rates: {line}', file=self.out)
        self.lib.wrnn_destroy(h)


def main():
    sections = ['plan', 'rate', 'rot', 'slice', 'bad', 'rates']
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--only', default=','.join(sections), help='comma-separated sections: ' + ', '.join(sections))
    args = ap.parse_args()
    d = Dump(sys.stdout)
    for s in args.only.split(','):
        if s not in sections:
            ap.error(f'unknown section {s}')
        getattr(d, s)()


if __name__ == '__main__':
    main()
