"""``bench.py --dump-outputs DIR``: what the timed path computed in its last step, written as ``DIR/<name>.npy`` so that two
builds of the project can be compared output for output (the inputs of a run depend on its arguments only)."""
import os

import numpy as np
import torch

DUMP_LIMIT_BYTES = 64_000_000          # everything written by one run
NPY_HEADER_BYTES = 4096                # per file, generous


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """Write every ``(name, tensor)`` of ``arrays`` as ``out_dir/<name>.npy``: float64 stays float64, every other type is written
    as float32. If the arrays hold more than ``limit`` bytes in all, each one larger than a single element is replaced by the
    same fraction of its elements: a seeded draw of positions of its flattened form (sorted, duplicates dropped), so two runs
    with the same arguments write the same positions. Returns ``{name: [elements written, elements of the output]}``."""
    os.makedirs(out_dir, exist_ok=True)
    items = []
    for name, t in arrays:
        t = torch.as_tensor(t).detach()
        items.append((name, t.to(torch.float64 if t.dtype == torch.float64 else torch.float32)))
    if any(t.is_cuda for _, t in items):
        torch.cuda.synchronize()                               # results of chains stepped on streams of their own included
    total = sum(t.numel() * t.element_size() for _, t in items)
    room = limit - NPY_HEADER_BYTES * len(items)
    frac = 1.0 if total <= room else room / total
    written = {}
    for k, (name, t) in enumerate(items):
        n = t.numel()
        if frac < 1.0 and n > 1:
            pos = np.unique(np.random.default_rng(seed + k).integers(0, n, size=max(int(n * frac), 1)))
            t = t.reshape(-1)[torch.from_numpy(pos).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())
        written[name] = [int(t.numel()), int(n)]
    return written
