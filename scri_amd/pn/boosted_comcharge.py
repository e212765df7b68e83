"""The post-Newtonian model of the boosted centre-of-mass charge (scri/pn/boosted_comcharge.py): what the reference's tutorial passes
to `map_to_superrest_frame` as `Gargsfun=PN_charges(m, nu)` and `Gfun=analytical_CoM_func` (docs/tutorial_abd.rst:419-522).

The PN parameter x = (m |omega|)^(2/3) comes from the angular velocity of the strain, `abd.h.angular_velocity()`, which is the GPU
`bms_angular_velocity`; everything after it is arithmetic on window-length arrays on the host, as `transformation_from_CoM_charge` is.
Energy and angular momentum: Blanchet, Living Reviews in Relativity 17 (2014), Eqs. (337), (338); the leading-order magnitude of the
centre-of-mass charge and the model time series: Khairnar et al., arXiv:2603.24661."""
import numpy as np


def PN_charges(m, ν):
    """(energy_pn, angular_momentum_pn, G_mag_pn, orbital_phase): callables of an `AsymptoticBondiData` object for a binary of total mass
    `m` and symmetric mass ratio `ν`, each returning its quantity at the object's time steps -- the energy to 2PN, the magnitude of the
    angular momentum to 3PN, the magnitude of the centre-of-mass charge at leading order, and the orbital phase from the (2, 1) mode of
    the strain.  Pass the tuple as `Gargsfun` to `map_to_superrest_frame`.

    The phase: SpEC's strain is minus the PN one and the leading (2, 1) amplitude carries a factor i, so ψ = -arg(-h_21) + π/2,
    unwrapped."""
    # coefficients of x^0, x^1, ... in the brackets of Eqs. (337) and (338)
    energy_series = (1.0, -3 / 4 - ν / 12, -27 / 8 + 19 / 8 * ν - ν**2 / 24)
    momentum_series = (1.0, 3 / 2 + ν / 6, -27 / 8 + 19 / 8 * ν - ν**2 / 24,
                       135 / 16 + (-6889 / 144 + 41 / 24 * np.pi**2) * ν + 31 / 24 * ν**2 + 7 / 1296 * ν**3)

    def pn_parameter(abd):
        Ω = np.asarray(abd.h.angular_velocity())
        return np.power(m * np.sqrt(np.einsum("ij,ij->i", Ω, Ω)), 2.0 / 3.0)

    def series(coefficients, x):
        total = coefficients[0] + coefficients[1] * x
        for k in range(2, len(coefficients)):
            total = total + coefficients[k] * x**k
        return total

    def energy_pn(abd):
        x = pn_parameter(abd)
        return m - (m * ν * x) / 2 * series(energy_series, x)

    def angular_momentum_pn(abd):
        x = pn_parameter(abd)
        return (m**2 * ν * x ** (-1 / 2)) * series(momentum_series, x)

    charge_scale = -1142 / 105 * np.sqrt(1 - 4 * ν) * (m * ν) ** 2  # leading order: G = charge_scale x^(5/2)

    def G_mag_pn(abd):
        return charge_scale * pn_parameter(abd) ** 2.5

    def orbital_phase(abd):
        h = abd.h
        h_21 = h.data[:, h.index(2, 1)]
        return np.unwrap(np.pi / 2 - np.angle(-h_21))

    return energy_pn, angular_momentum_pn, G_mag_pn, orbital_phase


def analytical_CoM_func(θ, t, E, J_mag, G_mag, ψ):
    """Model time series G[n, 3] of the boosted centre-of-mass charge over the frame-fixing window, for `Gfun` of
    `map_to_superrest_frame`: with β = θ[0:3] the boost velocity, X = θ[3:6] the translation, α1, α2 = θ[6:8] the two nuisance
    parameters, n = (cos ψ, sin ψ, 0), λ = (-sin ψ, cos ψ, 0) and J = J_mag z,

        G = (G_mag / E) (α1 λ + α2 n) - β x J / E - t β + X.

    t, E, J_mag, G_mag, ψ: arrays over the window (PN_charges)."""
    θ = np.asarray(θ)
    β, X = θ[0:3], θ[3:6]
    α1, α2 = θ[6:]
    cosψ, sinψ = np.cos(ψ), np.sin(ψ)
    ratio = G_mag / E
    spin = J_mag / E  # J / E has a z component only: β x J / E = (β_y, -β_x, 0) J_mag / E
    G = np.empty((np.shape(t)[0], 3))
    G[:, 0] = α1 * ratio * (-sinψ) + α2 * ratio * cosψ - β[1] * spin - t * β[0] + X[0]
    G[:, 1] = α1 * ratio * cosψ + α2 * ratio * sinψ + β[0] * spin - t * β[1] + X[1]
    G[:, 2] = -(t * β[2]) + X[2]
    return G
