"""Child process of tests/test_gemm_routes_gpu.py::test_every_row_takes_the_route_it_names: runs the case table of gemm_ref64 once, in
order, one capmi_gemm_f32 call per row, and prints the row names on stdout.  The parent starts it with CAPMI_GEMM_LOG=1 (read once
per process by libcapmi) and pairs the census lines on stderr with the names."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import torch                                            # noqa: E402

import gemm_ref64 as R                                  # noqa: E402
from imagecaptioning.pytorch_amd import ops             # noqa: E402


def main():
    dev = torch.device('cuda:0')
    ws = ops.Workspace(dev, R.WS_FLOATS)
    for c in R.CASES:
        R.run_case(c, R.to_device(R.draw(c), dev), ws)
        print(c['name'], flush=True)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
