# The host driver of the SRS view geometry (tests/test_srs_view_host.py): a plain build and one under the sanitizer flags of the
# Makefile beside it ($(SAN)), which this file includes rather than repeats.
#   make -f srs_view.mk srs_view_host srs_view_host_san
# (built beside the target and renamed into place: test processes that run side by side may build and run the same program)
include Makefile
SVDEPS = srs_view_host.cpp $(CSRC)/srs_view.hpp $(CSRC)/srs_policy.hpp $(CSRC)/srs_file.hpp $(CSRC)/proof_layout.hpp $(CSRC)/endo.hpp $(CSRC)/g1.hpp \
         $(CSRC)/field.hpp $(CSRC)/constants.hpp
srs_view_host: $(SVDEPS)
	$(CXX) -O1 -std=c++17 -Wall -Wextra -Wno-unknown-pragmas srs_view_host.cpp -o $@.$$$$.tmp && mv $@.$$$$.tmp $@
srs_view_host_san: $(SVDEPS)
	$(CXX) $(SAN) srs_view_host.cpp -o $@.$$$$.tmp && mv $@.$$$$.tmp $@
