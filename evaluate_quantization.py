#!/usr/bin/env python3
"""`python evaluate_quantization.py ...` -- same entry point and flags as the reference's evaluate_quantization.py; see
iswm_amd/evaluate_quantization.py."""
from iswm_amd.evaluate_quantization import main

if __name__ == "__main__":
    main()
