"""Writes the fixtures of tests/test_partition_ops.py from a checkout of the reference (rusty1s/pytorch_sparse):

    python tests/golden/make_partition_golden.py --reference PATH

  partition_weight2metis.npz   inputs and outputs of the reference's own weight2metis (torch_sparse/metis.py:10-21),
                               loaded from its source file at generation time (the function alone: importing the
                               package would need its compiled extension); `none_*` = 1 where it returns None
  partition_schemas.json       the schema strings torch gives the three ops of csrc/metis.cpp:18-69, taken from the
                               argument lists in that file
"""
import argparse
import ast
import json
import os
import re
from typing import Optional  # noqa: F401  (names the loaded function's annotations use)

import numpy as np
import torch
from torch import Tensor  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))

VECTORS = {
    'f32_small': torch.tensor([0.5, 1.0, 2.5, 0.5, 4.0], dtype=torch.float32),
    'f32_equal': torch.full((6,), 3.25, dtype=torch.float32),
    'f64_steps': torch.tensor([1.0, 1.125, 1.5, 3.0, 1.0, 2.25], dtype=torch.float64),
    'f32_random': torch.rand(64, generator=torch.Generator().manual_seed(0)),
    'f64_negative': torch.tensor([-2.0, 0.0, 6.0, 1.0], dtype=torch.float64),
    'f32_two': torch.tensor([1.0, 3.0], dtype=torch.float32),
}

TYPES = {'torch::Tensor': 'Tensor', 'std::optional<torch::Tensor>': 'Tensor?', 'int64_t': 'int', 'bool': 'bool'}


def load_weight2metis(reference):
    src = open(os.path.join(reference, 'torch_sparse', 'metis.py')).read()
    fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'weight2metis'][0]
    scope = {'torch': torch, 'Tensor': Tensor, 'Optional': Optional}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), 'metis.py', 'exec'), scope)
    return scope['weight2metis']


def schemas(reference):
    src = open(os.path.join(reference, 'csrc', 'metis.cpp')).read()
    out = {}
    for name in re.findall(r'\.op\("torch_sparse::(\w+)"', src):
        args = re.search(r'torch::Tensor\s+%s\((.*?)\)\s*\{' % name, src, re.S).group(1)
        kinds = [TYPES[' '.join(a.split()[:-1])] for a in args.split(',')]
        out[name] = 'torch_sparse::%s(%s) -> Tensor _0' % (name, ', '.join('%s _%d' % (t, i) for i, t in enumerate(kinds)))
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ref = ap.parse_args().reference
    w2m = load_weight2metis(ref)
    arrays = {}
    for name, vec in VECTORS.items():
        got = w2m(vec.clone())
        arrays['in_' + name] = vec.numpy()
        arrays['none_' + name] = np.array(int(got is None))
        arrays['out_' + name] = np.zeros(0, np.int64) if got is None else got.numpy()
    np.savez(os.path.join(HERE, 'partition_weight2metis.npz'), **arrays)
    with open(os.path.join(HERE, 'partition_schemas.json'), 'w') as fh:
        json.dump(schemas(ref), fh, indent=1, sort_keys=True)
        fh.write('\n')
