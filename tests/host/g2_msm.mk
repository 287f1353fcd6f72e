# The host driver of the G2 MSM's host-only parts (tests/test_g2_msm_host.py): a plain build and one under the sanitizer flags of the
# Makefile beside it ($(SAN)), which this file includes rather than repeats.   make -f g2_msm.mk g2_msm_host g2_msm_host_san
include Makefile
GDEPS = g2_msm_host.cpp $(wildcard $(CSRC)/*.hpp)
g2_msm_host: $(GDEPS)
	$(CXX) -O2 -std=c++17 -w g2_msm_host.cpp -o $@
g2_msm_host_san: $(GDEPS)
	$(CXX) $(SAN) g2_msm_host.cpp -o $@
