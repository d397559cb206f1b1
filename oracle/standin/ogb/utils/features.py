"""Sizes of the categorical atom / bond feature columns of ogb 1.3.2 (the last value of each column is 'misc')."""


def get_atom_feature_dims():
    # atomic number, chirality, degree, formal charge, number of Hs, radical electrons, hybridisation, aromatic, in ring
    return [119, 5, 12, 12, 10, 6, 6, 2, 2]


def get_bond_feature_dims():
    # bond type, stereo, conjugated
    return [5, 6, 2]
