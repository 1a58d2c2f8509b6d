"""Child process of tests/test_split_edges_gpu.py::test_register_staged_split16_form: started with GS_SPLIT16_DMA=0 (read once per
process), it runs the staged cases on split16_tiled_fwd_kernel through the same oracle checks and writes every output block to
the .npz named on the command line.  Not a test module."""
import os
import sys

import numpy as np
import torch


def main(path):
    assert os.environ.get("GS_SPLIT16_DMA") == "0", "this process must select the register-staged form"
    import test_split_edges_gpu as t
    dev = torch.device("cuda:0")
    res = t.staged_outputs(dev, "f16r")
    torch.cuda.synchronize()
    np.savez(path, **res)
    for k in sorted(t.WORST):
        print("worst err/bound %-24s %.4f" % (k, t.WORST[k]))


if __name__ == "__main__":
    main(sys.argv[1])
