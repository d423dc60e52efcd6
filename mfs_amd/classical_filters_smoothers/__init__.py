"""Classical filters, mirroring `mfs.classical_filters_smoothers`: the brute-force grid filter (the ground truth the moment
filters are measured against).  The particle and Gaussian filters of the reference's package are not here."""
