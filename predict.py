#!/usr/bin/env python3
"""`python predict.py ...` -- same entry point and flags as the reference's predict.py; see iswm_amd/predict.py."""
from iswm_amd.predict import main

if __name__ == "__main__":
    main()
