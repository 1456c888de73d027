"""Record the compiled reference's outputs (oracle/_ref, built by oracle/build_ref.py) on the cases of the tests that
compare the oracles with it, so that those tests also run where oracle/_ref cannot be built:

    ref_spmm.npz       test_oracle.test_c_oracle_matches_compiled_reference          (every dtype and reduction)
    ref_convert.npz    test_oracle.test_c_oracle_convert_matches_compiled_reference
    ref_value_bw.npz   test_oracle.test_c_oracle_value_bw_matches_compiled_reference
    ref_samplers.npz   test_oracle.test_np_oracle_matches_compiled_reference_samplers
    ref_schemas.json   test_ops_schema.test_schemas_equal_the_compiled_reference

The inputs are stored beside the outputs.  The cases come from the tests' own generators, at the smaller sizes
test_oracle.RECORDED_* name (the live comparison keeps the full ones).

    python tests/golden/make_ref_cases.py          (needs oracle/_ref)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref  # noqa: E402
from tests import test_oracle as to  # noqa: E402
from tests import test_ops_schema as ts  # noqa: E402
from tests.util import ALL_DTYPES, tonp  # noqa: E402


def save(name, arrays):
    path = os.path.join(HERE, 'ref_%s.npz' % name)
    np.savez_compressed(path, **arrays)
    print('wrote %s: %d arrays, %d bytes' % (path, len(arrays), os.path.getsize(path)))


def main():
    assert ref.available(), 'oracle/_ref is not built (python oracle/build_ref.py)'
    r = ref.ops()
    z = {}
    for dtype in ALL_DTYPES:
        rp, c, v, x = to.spmm_case_inputs(dtype, scale=to.RECORDED_SPMM_SCALE)
        z['spmm_rowptr'], z['spmm_col'] = rp.numpy(), c.numpy()
        name = to.dtype_name(dtype)
        z['spmm_%s_value' % name], z['spmm_%s_mat' % name] = tonp(v), tonp(x)
        for reduce in ('sum', 'mean', 'min', 'max'):
            for value, tag in ((v, 'val'), (None, 'noval')):
                ro, ra = to.ref_spmm(r, reduce, rp, c, value, x)
                z['spmm_%s_%s_%s_out' % (name, reduce, tag)] = ro
                if ra is not None:
                    z['spmm_%s_%s_%s_arg' % (name, reduce, tag)] = ra
    save('spmm', z)

    ind = to.convert_case_inputs()
    ptr = r.ind2ptr(ind, 300)
    save('convert', dict(convert_ind=ind.numpy(), convert_ptr=ptr.numpy(), convert_ind_back=r.ptr2ind(ptr, 2000).numpy()))

    z = {}
    for dtype in (torch.float32, torch.float64):
        row, rp, c, v, x, gout = to.value_bw_case_inputs(dtype, scale=to.RECORDED_VALUE_BW_SCALE)
        z['value_bw_row'], z['value_bw_rowptr'], z['value_bw_col'] = row.numpy(), rp.numpy(), c.numpy()
        key = 'value_bw_%s' % to.dtype_name(dtype)
        z[key + '_mat'], z[key + '_grad_out'] = tonp(x), tonp(gout)
        for reduce in ('sum', 'mean'):
            z['%s_%s_grad_value' % (key, reduce)] = to.ref_value_bw(r, reduce, row, rp, c, v, x, gout)
    save('value_bw', z)

    z = {}
    for seed in (0, 1, 2):
        a = to.sampler_case_inputs(seed, small=to.RECORDED_SAMPLER_SMALL)
        for k, v in a.items():
            z['samplers_%d_in_%s' % (seed, k)] = v
        for k, v in to.ref_samplers(r, seed, a).items():
            z['samplers_%d_%s' % (seed, k)] = v
    save('samplers', z)

    path = os.path.join(HERE, 'ref_schemas.json')
    with open(path, 'w') as fh:
        json.dump(ts.reference_schemas(), fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote %s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
